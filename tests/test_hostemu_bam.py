"""The device's BAM record encoder (chromap_amd/csrc/cm_bam.h) run by the host under emulated lanes (tests/hostemu/hostemu_bam.cpp)
against the plain-Python model (tests/bam_model.py): golden SAM lines put back into the stores' layout, and synthetic records at the
smallest shapes that can go wrong.  Every case runs with 8, 16 and 64 lanes in ascending and descending lane order; the bytes must be
the model's, the size function must say what was written, and nothing outside the records may be touched."""
import gzip
import os
import random

import pytest

import bam_model as bm
import hostemu_bam_lib as hb

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CONFIGS = [(G, rev) for G in (8, 16, 64) for rev in (False, True)]
_cache = {}


def _golden(case):
    if case not in _cache:
        path = os.path.join(GOLDEN, case)
        text = gzip.open(path, "rb").read()
        _cache[case] = (hb.store_from_sam(text), bm.encode(text)[1])
    return _cache[case]


def _check(st, want, G, rev, start=0, fills=(0x5A,)):
    """the encoder's bytes are `want`; with two fill patterns, every byte of them was written"""
    for fill in fills:
        got, off, refused = hb.encode(st, G, rev, start, fill)
        assert refused == 0
        assert off[-1] - off[0] == len(got) == len(want), "the size function and the model disagree"
        if got != want:
            at = next(i for i in range(len(want)) if got[i] != want[i])
            k = max(j for j in range(len(off)) if off[j] - start <= at)
            raise AssertionError("record %d, byte %d of it: %r, want %r" % (k, at - (off[k] - start), got[at:at + 8], want[at:at + 8]))
    return off


@pytest.mark.parametrize("case", ["s1_chip_sam.sam.gz", "s1_se_sam.sam.gz", "b1_bc_sam.sam.gz", "h1_hic_sam.sam.gz", "x2_gaps_sam_q0.sam.gz",
                                  "se_split/ss5_sam_q0.out.gz"])
def test_golden_lines_back_in_the_stores(case):
    st, want = _golden(case)
    assert len(st) > 100
    for k, (G, rev) in enumerate(CONFIGS):
        off = _check(st, want, G, rev, start=k % 4, fills=(0x5A, 0xA5) if k == 0 else (0x5A,))
    assert {o % 4 for o in off[:-1]} == {0, 1, 2, 3}
    assert any(r[10] == 0 for r in st.rec) and any(r[10] == 1 for r in st.rec), "both strands"
    assert (st.cb_len > 0) == case.startswith("b1_bc")


# ---- synthetic records: the expected SAM line is built here, field by field, and encoded by the model
REFS = [(b"c1", 1 << 28), (b"chrTwo", 1 << 28), (b"3", 70000)]
HEADER = b"".join(b"@SQ\tSN:%s\tLN:%d\n" % r for r in REFS)
SEQ_CHARS = b"ACGTacgtNnRYKMSWBDHVrykmswbdhv.=-xX@[`{"
NAME_LENS = [1, 3, 4, 5, 254]
QUALS = [33, 34, 126] + list(range(43, 126))  # (not 42: a QUAL column of "*" alone means no qualities)
NMS = [0, 255, 256, 65535, 65536]
MDS = [b"7", b"10A5", b"3^AC10T2", b"151"]  # 1 byte, multiples of 4, 3 bytes


def _cigar(kind, ql):
    """CIGAR words with query length ql"""
    M, I, D, S = 0, 1, 2, 4
    if kind == "many":  # 64 operations
        assert ql > 32
        ops = [(ql - 31, M)]
        for _ in range(31):
            ops += [(1, D), (1, M)]
        ops += [(2, D)]
        assert len(ops) == 64
    elif kind == "clip" and ql >= 4:
        ops = [(2, S), (ql - 3, M), (1, S)]
    elif kind == "del" and ql >= 2:
        ops = [(1, M), (5, D), (ql - 1, M)]
    elif kind == "ins" and ql >= 3:
        ops = [(1, M), (1, I), (ql - 2, M)]
    else:
        ops = [(ql, M)]
    assert sum(l for l, op in ops if op in (M, I, S)) == ql
    return [l << 4 | op for l, op in ops]


def _synthetic(cb_len, long_name_at=None):
    """(store, SAM text) of records that between them take every value of the table in the issue"""
    rng = random.Random(20 + cb_len)
    st = hb.Store(cb_len)
    lines = []
    k = 0
    for ql in (1, 2, 7, 8, 9, 151):
        for strand in (1, 0):
            for kind in ("plain", "clip", "del", "ins", "many"):
                if kind == "many" and ql != 151:
                    continue
                for trim_extra in ((0, 3, -1) if kind == "plain" else (k % 2 * 3,)):
                    if ql + trim_extra < 1:
                        continue
                    words = _cigar(kind, ql)
                    trim_len = ql + trim_extra
                    sl = min(ql, trim_len)
                    ref_len = sum(w >> 4 for w in words if w & 15 in (0, 2, 3, 7, 8))
                    name_len = NAME_LENS[k % 5] if long_name_at != k else 255
                    name = bytes(rng.choice(b"abcXYZ019_:/") for _ in range(name_len))
                    read = bytes(rng.choice(SEQ_CHARS) for _ in range(trim_len + 2))
                    qual = bytes(rng.choice(QUALS) for _ in range(trim_len + 2))
                    rid = k % 3
                    # an alignment that ends exactly at a 16 kb boundary, one that ends one base past it, and others
                    pos = [16384 * 3 - ref_len, 16384 * 3 - ref_len + 1, 0, 131072 - 1, rng.randrange(1 << 27)][k % 5]
                    if rid == 2:
                        pos %= 60000
                    mrid = [-1, rid, (rid + 1) % 3][(k // 3) % 3]
                    mpos = rng.randrange(60000)
                    tlen = [0, -rng.randrange(1, 1000), rng.randrange(1, 1 << 20), -(1 << 27)][k % 4] if mrid >= 0 else 0
                    flag = (0 if strand else 16) | [0, 1 | 64, 1 | 128 | 32][k % 3]
                    mapq, nm, md = [0, 1, 30, 60, 255][(k // 3) % 5], NMS[(k // 5 + k) % 5], MDS[(k // 2 + k) % 4]
                    barcode = bytes(rng.choice(b"ACGT") for _ in range(cb_len)) if cb_len else None
                    st.add(rid, pos, mrid, mpos, tlen, flag, mapq, nm, words, md, name, read, qual, strand, trim_len, barcode)
                    if strand:
                        seq, q = read[:sl], qual[:sl]
                    else:  # the SAM line's bases: the reverse complement of the last sl of the first trim_len
                        seq, q = hb.revcomp(read[trim_len - sl:trim_len]), qual[trim_len - sl:trim_len][::-1]
                    cig = "".join("%d%s" % (w >> 4, "MIDNSHP=X"[w & 15]) for w in words).encode()
                    rnext = b"*" if mrid < 0 else b"=" if mrid == rid else REFS[mrid][0]
                    cols = [name, b"%d" % flag, REFS[rid][0], b"%d" % (pos + 1), b"%d" % mapq, cig, rnext, b"%d" % (mpos + 1 if mrid >= 0 else 0),
                            b"%d" % tlen, seq, q, b"NM:i:%d" % nm, b"MD:Z:" + md] + ([b"CB:Z:" + barcode] if cb_len else [])
                    if long_name_at != k:
                        lines.append(b"\t".join(cols) + b"\n")
                    k += 1
    return st, HEADER + b"".join(lines)


@pytest.mark.parametrize("cb_len", [0, 16])
def test_synthetic_records(cb_len):
    st, sam = _synthetic(cb_len)
    want = bm.encode(sam)[1]
    rows = [ln.split(b"\t") for ln in sam.split(b"\n") if ln and not ln.startswith(b"@")]
    # the table of shapes is covered
    assert {len(r[9]) for r in rows} >= {1, 2, 7, 8, 9, 151} and {len(r[0]) for r in rows} == {1, 3, 4, 5, 254}
    for sl in (1, 2, 7, 8, 9, 151):
        assert {int(r[1]) & 16 for r in rows if len(r[9]) == sl} == {0, 16}
    assert {int(r[11][5:]) for r in rows} == set(NMS)
    assert {r[7] for r in st.rec} >= {1, 64} and {r[8] for r in st.rec} >= {1, 4, 8}
    assert any(b"S" in r[5] for r in rows) and any(b"D" in r[5] for r in rows)
    assert {r[6] for r in rows} == {b"*", b"=", b"c1", b"chrTwo", b"3"} and any(int(r[8]) < 0 for r in rows)
    assert any(set(r[9]) & set(b"acgt") for r in rows) and any(set(r[9]) & set(b"RYKM") for r in rows) and any(b"." in r[9] for r in rows)
    ends = {(r[1] + sum(w >> 4 for w in st.cigar[st.cigar_off[i]:st.cigar_off[i + 1]] if w & 15 in (0, 2))) % 16384 for i, r in enumerate(st.rec)}
    assert {0, 1} <= ends, "an alignment ends at a 16 kb boundary, another one base past it"
    assert bm.decode(bm.encode(sam)[0] + want) == bm.normalise(sam)
    for k, (G, rev) in enumerate(CONFIGS):
        for start in range(4):
            off = _check(st, want, G, rev, start=start, fills=(0x5A, 0xA5) if start == k % 4 else (0x5A,))
    assert {o % 4 for o in off[:-1]} == {0, 1, 2, 3}, "records start at all four offsets mod 4"


@pytest.mark.parametrize("G,rev", CONFIGS)
def test_a_name_of_255_bytes_is_refused(G, rev):
    st, sam = _synthetic(16, long_name_at=7)
    assert max(st.name_off[i + 1] - st.name_off[i] for i in range(len(st))) == 255
    got, off, refused = hb.encode(st, G, rev)
    assert refused == 1 and off[8] == off[7], "counted, and no byte of it"
    assert got == bm.encode(sam)[1], "the other records are written as if it were not there"


def test_codes_and_words_equal_the_model():
    L = hb.lib()
    for c in range(256):
        ch = chr(c).upper()
        assert L.hostemu_bam_code(c, 0) == (bm.SEQ_ALPHABET.index(ch) if ch in bm.SEQ_ALPHABET else 15), c
        comp = {"A": "T", "C": "G", "G": "C", "T": "A"}.get(ch, "N")
        assert L.hostemu_bam_code(c, 1) == bm.SEQ_ALPHABET.index(comp), c
    rng = random.Random(5)
    for x in [0, 0xffffffff, 0x21212121, 0x20202020, 0x7e21ff00] + [rng.getrandbits(32) for _ in range(2000)]:
        want = sum((((x >> s & 0xff) - 33) & 0xff) << s for s in (0, 8, 16, 24))
        assert L.hostemu_bam_sub33(x) == want, hex(x)
    for shift in (14, 17, 20, 23, 26):
        for beg in ((1 << shift) - 2, (1 << shift) - 1, 1 << shift, 3 << shift):
            for ln in (1, 2, 1 << shift):
                assert L.hostemu_bam_reg2bin(beg, beg + ln) == bm.reg2bin(beg, beg + ln)
    assert L.hostemu_bam_reg2bin(0, 1) == 4681
