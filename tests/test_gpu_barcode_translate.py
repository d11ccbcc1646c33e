"""--barcode-translate on the device (cm_barcode_translate.h; cm_post.hip: column 4 of the barcoded BED kinds; cm_sam_post.hip: the
CB:Z: value).  The expected text never comes from the code under test: it is the text the same store gives WITHOUT a table, with
column 4 replaced by a Python model of the reference's Translate (barcode_translator.h:73-100: segments cut with its shifts on 64-bit
values, joined with '-').  For SAM and the command line the expectation is the host route / the run without the flag."""
import ctypes as C
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import datasets
import oracle_lib as ol

pytestmark = pytest.mark.gpu
CLI = os.path.join(datasets.ROOT, "chromap_amd", "chromap-amd")
REF = os.path.join(datasets.ROOT, "oracle", "_ref", "chromap")
EFORMAT = -7
MISS = "Barcode does not exist in the translation table."
M64 = (1 << 64) - 1


# ---- the model
def key_of(seq):
    k = 0
    for ch in seq:
        k = (k << 2) | {65: 0, 67: 1, 71: 2, 84: 3}.get(ch & 0xDF, 0)
    return k & M64


def seq_of(key, n):
    return bytes(b"ACGT"[(key >> (2 * (n - 1 - j))) & 3] for j in range(n))


def parse_table(text):
    table, from_len = {}, 0
    for line in text.split(b"\n"):
        seps = [i for i, c in enumerate(line) if c in b",\t"]
        if seps:
            from_len = len(line) - seps[0] - 1
            table[key_of(line[seps[0] + 1:])] = line[:seps[0]]
    return table, from_len


def model_translate(table, from_len, key, bc_len):
    n = bc_len // from_len
    mask = M64 if from_len >= 32 else (1 << (2 * from_len)) - 1
    out = []
    for i in range(n):
        seed = (((key << (2 * i * from_len)) & M64) >> (2 * (n - 1) * from_len)) & mask
        if seed not in table:
            return None
        out.append(table[seed])
    return b"-".join(out)


def translate_bed(plain, table_text, bc_len):
    """column 4 of every line of `plain` through the model"""
    table, from_len = parse_table(table_text)
    out = []
    for line in plain.split(b"\n")[:-1]:
        c = line.split(b"\t")
        assert len(c) == 5 and len(c[3]) == bc_len
        c[3] = model_translate(table, from_len, key_of(c[3]), bc_len)
        assert c[3] is not None
        out.append(b"\t".join(c) + b"\n")
    return b"".join(out)


# ---- records
def make_records(rng, n, barcodes, n_seq=3, span=40):
    from chromap_amd.distributed import REC_DTYPE
    rb = np.zeros(n, np.dtype([("r", REC_DTYPE), ("barcode", "<u8")]))
    r = rb["r"]
    r["read_id"] = rng.permutation(n).astype(np.uint32)
    r["rid"] = rng.integers(0, n_seq, n)
    r["fragment_start"] = rng.integers(10, 10 + span, n)
    r["fragment_length"] = rng.integers(30, 33, n)
    r["mapq"] = rng.choice([0, 1, 3, 30, 60], n)
    r["direction"] = rng.integers(0, 2, n)
    r["is_unique"] = rng.integers(0, 2, n)
    r["num_dups"] = 1
    r["positive_alignment_length"] = rng.integers(20, 60, n)
    r["negative_alignment_length"] = rng.integers(20, 60, n)
    # half of the records share six barcodes: cell-level duplicate runs
    pick = np.where(rng.random(n) < 0.5, rng.integers(0, min(6, len(barcodes)), n), rng.integers(0, len(barcodes), n))
    rb["barcode"] = np.asarray(barcodes, np.uint64)[pick]
    return rb


def make_table(rng, n_entries, from_len, name_len, prefix=b""):
    """(text, keys): n_entries distinct keys of from_len bases; name_len(i) -> the length of entry i's name"""
    keys = set()
    while len(keys) < min(n_entries, 4 ** from_len):
        keys.add(int(rng.integers(0, 4 ** min(from_len, 31), dtype=np.uint64)))
    keys = sorted(keys)
    lines = []
    for i, k in enumerate(keys):
        ln = name_len(i)
        name = (prefix + b"%d_" % i + bytes(97 + (i + j) % 26 for j in range(ln)))[:ln]
        lines.append(name + (b"\t" if i & 1 else b",") + seq_of(k, from_len))
    return b"\n".join(lines) + b"\n", keys


@pytest.fixture(scope="module")
def gpu():
    from chromap_amd import ChromapGPU
    fa, _, _ = datasets.case_inputs("toy_chip")
    g = ChromapGPU(datasets.case_index("toy_chip"), fa, preset="chip")
    g.names = [b"seq%d" % i for i in range(3)]
    yield g
    g.close()


def text_bytes(g):
    nb = C.c_uint64(7)
    assert g.L.cmgpu_store_info(g.ctx, None, C.byref(nb), None) == 0
    return nb.value


def fill(g, rb):
    g.store_clear()
    g.store_append(rb.ctypes.data, len(rb), barcoded=True)


def plain_and_translated(g, kind, p, bc_len, table_text):
    """(text without a table, text with it, (lines, bytes) the translated call reported)"""
    g.set_barcode_translation(None)
    g.store_format(kind, params=p, barcode_length=bc_len)
    plain = g.store_text()
    g.set_barcode_translation(table_text)
    counts = g.store_format(kind, params=p, barcode_length=bc_len)
    got = g.store_text()
    g.set_barcode_translation(None)
    return plain, got, counts


MODES = [(lowmem, dedup, tn5) for lowmem in (1, 0) for dedup in (1, 0) for tn5 in (1, 0)]


# ---- 1. plain
@pytest.mark.parametrize("kind", [2, 5], ids=["pe_bc", "se_bc"])
def test_short_names_every_mode(gpu, kind):
    from chromap_amd import _capi
    rng = np.random.default_rng(11 + kind)
    table_text, keys = make_table(rng, 300, 16, lambda i: i % 41)
    assert gpu.barcode_translation_info() == (0, 0, 0)
    rb = make_records(rng, 5000, keys)
    fill(gpu, rb)
    seen = set()
    for lowmem, dedup, tn5 in MODES:
        p = _capi.default_params(None, remove_pcr_duplicates=dedup, low_memory_mode=lowmem, tn5_shift=tn5, mapq_threshold=1)
        plain, got, (lines, nbytes) = plain_and_translated(gpu, kind, p, 16, table_text)
        want = translate_bed(plain, table_text, 16)
        assert got == want
        assert nbytes == len(want) and lines == want.count(b"\n") and lines > 1000
        seen.add(want)
    assert len(seen) >= 4  # the modes differ (duplicate removal, its two rules, the shift)
    gpu.set_barcode_translation(table_text)
    n, fl, hbm = gpu.barcode_translation_info()
    assert (n, fl) == (300, 16) and hbm == 1024 * 16 + sum(i % 41 for i in range(300))
    gpu.set_barcode_translation(None)
    assert gpu.barcode_translation_info() == (0, 0, 0)


# ---- 2. long names: lines that do not fit the LDS staging of a 256-line block
@pytest.mark.parametrize("mixed", [False, True], ids=["long", "short_and_long"])
@pytest.mark.parametrize("kind", [2, 5], ids=["pe_bc", "se_bc"])
def test_long_names(gpu, kind, mixed):
    from chromap_amd import _capi
    rng = np.random.default_rng(23 + kind + 2 * mixed)
    # (a table line stays under 512 bytes, the reference's gzgets buffer: name + separator + 16 bases + newline)
    length = (lambda i: 200 + (i * 37) % 291 if i % 3 == 0 else i % 11) if mixed else (lambda i: 200 + (i * 37) % 291)
    table_text, keys = make_table(rng, 300, 16, length)
    assert max(len(ln) for ln in table_text.split(b"\n")) < 511
    rb = make_records(rng, 5000, keys)
    if mixed:  # barcodes uniform over the table: a third of the lines are long
        rb["barcode"] = np.asarray(keys, np.uint64)[rng.integers(0, len(keys), len(rb))]
    fill(gpu, rb)
    for lowmem, dedup, tn5, q in [(1, 0, 0, 0), (1, 1, 1, 1), (0, 1, 1, 30), (0, 0, 1, 0)]:
        p = _capi.default_params(None, remove_pcr_duplicates=dedup, low_memory_mode=lowmem, tn5_shift=tn5, mapq_threshold=q)
        plain, got, (lines, nbytes) = plain_and_translated(gpu, kind, p, 16, table_text)
        want = translate_bed(plain, table_text, 16)
        assert got == want
        assert nbytes == len(want) and lines == want.count(b"\n")
        if not dedup and q == 0:
            # every record is a line here, so block b of the format kernel holds lines 256 b .. 256 b + 255: which blocks are
            # staged in LDS (at most 32768 bytes) and which write to the text directly is known
            ln = [len(x) + 1 for x in want.split(b"\n")[:-1]]
            assert len(ln) == 5000
            sizes = [sum(ln[i:i + 256]) for i in range(0, 5000, 256)]
            direct = sum(s > 32768 for s in sizes)
            assert direct == len(sizes) if not mixed else 0 < direct < len(sizes), sizes


# ---- 3. segments
@pytest.mark.parametrize("bc_len,from_len", [(16, 8), (12, 4), (16, 5), (16, 20), (32, 16), (32, 32)])
def test_segments(gpu, bc_len, from_len):
    from chromap_amd import _capi
    rng = np.random.default_rng(100 * bc_len + from_len)
    table_text, keys = make_table(rng, 50, from_len, lambda i: (i * 7) % 23, prefix=b"s")
    n = bc_len // from_len
    rem = bc_len - n * from_len
    barcodes = []
    for _ in range(40):
        # the reference's shifts read the LOW n * from_len bases; what stands above them (bc_len no multiple of from_len) is ignored
        k = int(rng.integers(0, 4 ** rem)) if rem else 0
        for _ in range(n):
            k = (k << (2 * from_len)) | keys[int(rng.integers(0, len(keys)))]
        if n == 0:
            k = int(rng.integers(0, 4 ** bc_len, dtype=np.uint64))
        barcodes.append(k)
    rb = make_records(rng, 3000, barcodes)
    fill(gpu, rb)
    p = _capi.default_params(None, remove_pcr_duplicates=1, low_memory_mode=1, tn5_shift=1, mapq_threshold=1)
    for kind in (2, 5):
        plain, got, (lines, nbytes) = plain_and_translated(gpu, kind, p, bc_len, table_text)
        want = translate_bed(plain, table_text, bc_len)
        assert got == want and nbytes == len(want) and lines == want.count(b"\n") and lines > 500
        col = [ln.split(b"\t")[3] for ln in want.split(b"\n")[:-1]]
        if n == 0:
            assert set(col) == {b""}  # the table's `from` is longer than the barcode: an empty column
        else:
            assert all(c.count(b"-") >= n - 1 for c in col)


# ---- 4. the miss rule
def raw_format(g, kind, p, bc_len):
    names = (C.c_char_p * len(g.names))(*g.names)
    nl, nb = C.c_uint64(0), C.c_uint64(0)
    rc = g.L.cmgpu_store_format(g.ctx, kind, names, len(g.names), C.byref(p), bc_len, C.byref(nl), C.byref(nb))
    return rc, nl.value, nb.value


def test_a_miss_counts_only_for_a_line_that_would_be_printed(gpu):
    from chromap_amd import ChromapError, _capi
    rng = np.random.default_rng(404)
    table_text, keys = make_table(rng, 300, 16, lambda i: 3 + i % 9)
    absent = next(k for k in range(1, 1000) if k not in keys)
    rb = make_records(rng, 2000, keys)
    rb["r"]["mapq"] = 60
    odd = 777
    rb["barcode"][odd] = absent
    rb["r"]["rid"][odd], rb["r"]["fragment_start"][odd], rb["r"]["fragment_length"][odd] = 1, 5000, 31  # a position of its own
    cell = _capi.default_params(None, remove_pcr_duplicates=1, low_memory_mode=1, tn5_shift=0, mapq_threshold=30)
    # (a) it survives
    fill(gpu, rb)
    gpu.set_barcode_translation(table_text)
    for kind in (2, 5):
        rc, nl, nb = raw_format(gpu, kind, cell, 16)
        assert rc == EFORMAT and (nl, nb) == (0, 0)
        assert gpu.L.cmgpu_last_error(gpu.ctx).decode() == MISS
        assert text_bytes(gpu) == 0 and gpu.store_text() == b""
        with pytest.raises(ChromapError, match=re.escape(MISS)):
            gpu.store_format(kind, params=cell, barcode_length=16)
    # ... and the error does not wedge the context: without the table the plain text comes back, with it and without the record
    # the translated one
    gpu.set_barcode_translation(None)
    gpu.store_format(2, params=cell, barcode_length=16)
    plain_with_odd = gpu.store_text()
    assert seq_of(absent, 16) in plain_with_odd
    keep = np.ones(len(rb), bool)
    keep[odd] = False
    fill(gpu, rb[keep].copy())
    plain, got, _ = plain_and_translated(gpu, 2, cell, 16, table_text)
    assert got == translate_bed(plain, table_text, 16)
    assert plain == b"".join(ln + b"\n" for ln in plain_with_odd.split(b"\n")[:-1] if seq_of(absent, 16) not in ln)
    # (b) its MAPQ is below -q
    rb["r"]["mapq"][odd] = 3
    fill(gpu, rb)
    plain_b, got_b, (lines, nbytes) = plain_and_translated(gpu, 2, cell, 16, table_text)
    assert plain_b == plain and got_b == got and nbytes == len(got) and lines == got.count(b"\n")
    rb["r"]["mapq"][odd] = 60
    # (c) it is the losing member of a duplicate run.  A cell-level run has one barcode, so this is a bulk-level run (same rid, start
    # and length whatever the barcode): a barcode group of two records beats the single record with the absent barcode
    bulk = _capi.default_params(None, remove_pcr_duplicates=1, low_memory_mode=1, tn5_shift=0, mapq_threshold=30, dedup_at_bulk_level=1)
    wl = np.ascontiguousarray(np.asarray(keys + [absent], np.uint64))
    assert gpu.L.cmgpu_set_whitelist(gpu.ctx, wl.ctypes.data, len(wl), 16) == 0
    gpu.barcode_length = 16
    sample = b"".join(seq_of(int(k), 16) for k in wl)
    gpu.compute_barcode_abundance(np.frombuffer(sample, np.uint8), np.arange(0, len(sample) + 1, 16, dtype=np.uint32))
    rc2 = rb.copy()
    for t in (100, 101):  # two records of one listed barcode at the odd record's position
        rc2["r"]["rid"][t], rc2["r"]["fragment_start"][t], rc2["r"]["fragment_length"][t] = 1, 5000, 31
        rc2["barcode"][t] = keys[5]
    fill(gpu, rc2)
    plain_c, got_c, (lines, nbytes) = plain_and_translated(gpu, 2, bulk, 16, table_text)
    assert got_c == translate_bed(plain_c, table_text, 16) and nbytes == len(got_c) and lines == got_c.count(b"\n")
    assert b"seq1\t5000\t5031\t" + seq_of(keys[5], 16) + b"\t3\n" in plain_c and seq_of(absent, 16) not in plain_c
    # the same run without the two: the absent barcode survives, and the call fails
    fill(gpu, rb)
    gpu.set_barcode_translation(table_text)
    assert raw_format(gpu, 2, bulk, 16)[0] == EFORMAT
    gpu.set_barcode_translation(None)


# ---- 5. inertness
def test_kinds_without_a_barcode_column_ignore_the_table_and_the_table_can_be_copied(gpu):
    from chromap_amd import ChromapGPU, _capi
    rng = np.random.default_rng(55)
    table_text, keys = make_table(rng, 300, 16, lambda i: 250 if i % 3 == 0 else i % 30)
    rb = make_records(rng, 4000, keys)
    p = _capi.default_params(None, remove_pcr_duplicates=1, low_memory_mode=1, tn5_shift=1, mapq_threshold=1)
    bulk_rec = np.ascontiguousarray(rb["r"])

    def texts(kinds, barcoded):
        out = []
        for kind in kinds:
            nl, nb = gpu.store_format(kind, params=p, barcode_length=16 if barcoded else 0)
            out.append((nl, nb, gpu.store_text()))
        return out
    gpu.store_clear()
    gpu.store_append(bulk_rec.ctypes.data, len(bulk_rec))
    without = texts((0, 1, 3), False)
    gpu.set_barcode_translation(table_text)
    assert texts((0, 1, 3), False) == without and all(t[0] > 100 for t in without)
    gpu.set_barcode_translation(None)
    fill(gpu, rb)
    without = texts((4, 6, 2, 5), True)
    gpu.set_barcode_translation(table_text)
    with_table = texts((4, 6, 2, 5), True)
    assert with_table[:2] == without[:2] and all(t[0] > 100 for t in without)  # TagAlign PE_BC and SE_BC
    for (_, _, plain), (nl, nb, got) in zip(without[2:], with_table[2:]):
        want = translate_bed(plain, table_text, 16)
        assert got == want and got != plain and nb == len(want) and nl == want.count(b"\n")
    # the table copied into a context made by cmgpu_create_shared formats identically
    child = ChromapGPU(shared_from=gpu)
    try:
        assert child.barcode_translation_info() == (0, 0, 0)
        assert gpu.L.cmgpu_copy_barcode_translation(child.ctx, gpu.ctx) == 0
        assert child.barcode_translation_info() == gpu.barcode_translation_info() and child.barcode_translation_info()[0] == 300
        child.store_append(rb.ctypes.data, len(rb), barcoded=True)
        assert child.store_format(2, params=p, barcode_length=16) == with_table[2][:2]
        assert child.store_text() == with_table[2][2]
        gpu.set_barcode_translation(None)  # (the child's is a copy: it stays)
        assert child.store_format(5, params=p, barcode_length=16) == with_table[3][:2]
        assert child.store_text() == with_table[3][2]
        assert gpu.L.cmgpu_copy_barcode_translation(child.ctx, gpu.ctx) == 0  # a source without a table clears
        assert child.barcode_translation_info() == (0, 0, 0)
        child.store_format(2, params=p, barcode_length=16)
        assert child.store_text() == without[2][2]
    finally:
        child.close()
    # set(None) restores the plain barcoded text
    assert texts((2, 5), True) == without[2:]


# ---- 6. SAM: the CB:Z: value
def run_cli(args, out, ok=True):
    r = subprocess.run([CLI] + list(args) + ["-o", out], stderr=subprocess.PIPE)
    if ok:
        assert r.returncode == 0, r.stderr.decode()[-1500:]
    return r


def whitelist_table(wlf, path, name=lambda i: "CELL%05d%s" % (i, "x" * (i % 37)), skip=(), gz=False):
    with open(wlf) as f, (gzip.open(path, "wt") if gz else open(path, "w")) as t:
        for i, ln in enumerate(f):
            if ln.strip() and ln.strip() not in skip:
                t.write("%s%s%s\n" % (name(i), "\t" if i & 1 else ",", ln.strip()))
    return path


def test_sam_cb_value_equals_the_host_route(tmp_path):
    from chromap_amd import ChromapError, ChromapGPU, Stats
    case = datasets.SAM_BC_CASES[0]
    meta = datasets.case_meta(case)
    fa, r1, r2 = datasets.case_inputs(case)
    bcf, wlf = datasets.case_barcode_inputs(case)
    idx = datasets.case_index(case)
    table = whitelist_table(wlf, str(tmp_path / "tr.tsv"))
    want = str(tmp_path / "host.sam")
    run_cli(list(meta["chromap_flags"]) + ["--barcode-translate", table, "-x", idx, "-r", fa, "-1", r1, "-2", r2, "-b", bcf, "--barcode-whitelist", wlf], want)
    want = open(want, "rb").read()
    assert b"CB:Z:CELL" in want
    preset, kw = datasets.flags_to_params(meta["chromap_flags"])
    g = ChromapGPU(idx, fa, preset=preset, **kw)
    try:
        g.fastq_keep_reads(True)
        n = g.fastq_scan(0, open(r1, "rb").read(), True)
        assert g.fastq_scan(1, open(r2, "rb").read(), True) == n
        bc, _, bco = ol.read_fastq_qual(bcf)
        bc_len = int(bco[1] - bco[0])
        g.set_whitelist_file(wlf, bc_len)
        g.compute_barcode_abundance(bc, bco)
        assert g.fastq_scan(2, open(bcf, "rb").read(), True) == n
        for s in (2, 0, 1):
            g.fastq_take(s, n)
        g.fastq_commit(n, first_read_id=0, paired=True, barcoded=True)
        g.map_resident(Stats())
        g.sam_store_clear()
        assert g.sam_store_append_resident() > 100
        for group in (8, 16, 64):
            g.set_option("sam_format_group", group)
            g.set_barcode_translation(table)  # (a path)
            lines, nbytes = g.store_format_sam(barcode_length=bc_len)
            out = str(tmp_path / "dev.sam")
            g.write_sam_header(out)
            g.store_write_text(out, append=True)
            got = open(out, "rb").read()
            assert got == want
            assert lines == sum(1 for ln in want.split(b"\n") if ln and not ln.startswith(b"@SQ"))
            assert nbytes == sum(len(ln) + 1 for ln in want.split(b"\n") if ln and not ln.startswith(b"@SQ"))
        # a table that lacks most barcodes
        g.set_barcode_translation(open(table, "rb").read().split(b"\n")[0] + b"\n")
        with pytest.raises(ChromapError, match=re.escape(MISS)):
            g.store_format_sam(barcode_length=bc_len)
        assert text_bytes(g) == 0
        g.set_barcode_translation(None)
        lines2, _ = g.store_format_sam(barcode_length=bc_len)
        out = str(tmp_path / "plain.sam")
        g.write_sam_header(out)
        g.store_write_text(out, append=True)
        assert open(out, "rb").read() == datasets.case_golden_bed(case) and lines2 == lines
    finally:
        g.close()


# ---- 7. the command line
def cli_case(tmp_path):
    case = "b1_atac_bc"
    fa, r1, r2 = datasets.case_inputs(case)
    bcf, wlf = datasets.case_barcode_inputs(case)
    common = list(datasets.case_meta(case)["chromap_flags"]) + ["-x", datasets.case_index(case), "-r", fa, "-1", r1, "-2", r2, "-b", bcf,
                                                              "--barcode-whitelist", wlf]
    return case, common, wlf


def formatted_bytes(stderr):
    m = re.search(rb"Sorted, deduplicated and formatted (\d+) bytes", stderr)
    assert m, stderr.decode()[-1500:]
    return int(m.group(1))


def CELL_NAME(i):  # no name is as long as the barcode
    return "C%d" % i if i % 3 else "a_rather_longer_name_for_cell_%d" % i


@pytest.fixture(scope="module")
def cli_plain(tmp_path_factory):
    """the run without the flag, once: (arguments, whitelist, BED text, --summary CSV, table, the same table gzip-compressed, the
    Python translation of the BED text)"""
    d = tmp_path_factory.mktemp("cli_plain")
    case, common, wlf = cli_case(d)
    run_cli(common + ["--summary", str(d / "plain.csv")], str(d / "plain.bed"))
    plain = open(str(d / "plain.bed"), "rb").read()
    assert plain == datasets.case_golden_bed(case)
    table = whitelist_table(wlf, str(d / "tr.tsv"), CELL_NAME)
    table_gz = whitelist_table(wlf, str(d / "tr.tsv.gz"), CELL_NAME, gz=True)
    want = translate_bed(plain, open(table, "rb").read(), len(plain.split(b"\t")[3]))
    assert len(want) != len(plain)
    return common, wlf, plain, open(str(d / "plain.csv"), "rb").read(), table, table_gz, want


@pytest.mark.parametrize("variant", ["plain_table", "force_exchange", "gzip_table"])
def test_cli_translates_bed_on_the_device(cli_plain, variant, tmp_path):
    common, wlf, plain, plain_csv, table, table_gz, want = cli_plain
    extra = {"plain_table": ["--barcode-translate", table], "force_exchange": ["--barcode-translate", table, "--force-exchange"],
             "gzip_table": ["--barcode-translate", table_gz]}[variant]
    out, csv = str(tmp_path / "t.bed"), str(tmp_path / "t.csv")
    r = run_cli(common + extra + ["--summary", csv], out)
    assert open(out, "rb").read() == want
    assert formatted_bytes(r.stderr) == os.path.getsize(out) == len(want)  # the size of the translated text, which is the file's
    assert open(csv, "rb").read() == plain_csv                             # --summary prints Seed2Sequence: a table changes nothing


def test_cli_table_that_lacks_a_barcode_of_the_output(cli_plain, tmp_path):
    common, wlf, plain, _, _, _, _ = cli_plain
    used = plain.split(b"\n")[len(plain.split(b"\n")) // 2].split(b"\t")[3].decode()
    short = whitelist_table(wlf, str(tmp_path / "short.tsv"), CELL_NAME, skip=(used,))
    r = run_cli(common + ["--barcode-translate", short], str(tmp_path / "miss.bed"), ok=False)
    assert r.returncode != 0 and MISS.encode() in r.stderr


def test_cli_translated_bed_equals_the_reference_binary(tmp_path):
    if not os.path.exists(REF):
        pytest.skip("built reference binary not present")
    case, common, wlf = cli_case(tmp_path)
    table = whitelist_table(wlf, str(tmp_path / "tr.tsv"), CELL_NAME)
    out_ref, out_gpu = str(tmp_path / "r.bed"), str(tmp_path / "g.bed")
    subprocess.run([REF] + common + ["--barcode-translate", table, "-o", out_ref, "-t", "16"], check=True, stderr=subprocess.PIPE)
    run_cli(common + ["--barcode-translate", table], out_gpu)
    assert open(out_gpu, "rb").read() == open(out_ref, "rb").read()
