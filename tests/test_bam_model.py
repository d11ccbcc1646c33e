"""tests/bam_model.py against itself and against the definition of the bins: decode(encode(x)) is x for every committed SAM golden
file, and reg2bin is the smallest bin of the five-level scheme that contains the interval."""
import glob
import gzip
import os
import struct

import pytest

import bam_model as bm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SAM_FILES = sorted(glob.glob(os.path.join(GOLDEN, "*_sam*.sam.gz")) + glob.glob(os.path.join(GOLDEN, "summary", "*_sam*.sam.gz")) +
                   [os.path.join(GOLDEN, "se_split", "ss5_sam_q0.out.gz"), os.path.join(GOLDEN, "cli_only", "c7_sam_barcode_translate.out.gz")])


def test_there_are_golden_sam_files():
    names = [os.path.basename(f) for f in SAM_FILES]
    assert len(names) >= 12 and "s1_chip_sam.sam.gz" in names and "b1_bc_sam.sam.gz" in names and "ss5_sam_q0.out.gz" in names


@pytest.mark.parametrize("path", SAM_FILES, ids=[os.path.relpath(f, GOLDEN) for f in SAM_FILES])
def test_decode_of_encode_is_the_text(path):
    text = gzip.open(path, "rb").read()
    lines = [ln for ln in text.split(b"\n") if ln and not ln.startswith(b"@")]
    assert len(lines) > 100
    header, records = bm.encode(text)
    assert header[:4] == b"BAM\1"
    assert bm.decode(header + records) == bm.normalise(text)
    # the records are as long as their fields say, back to back
    at, n = 0, 0
    while at < len(records):
        at += 4 + struct.unpack_from("<I", records, at)[0]
        n += 1
    assert at == len(records) and n == len(lines)


def test_the_alphabet_and_the_tags():
    sam = (b"@SQ\tSN:c1\tLN:100000\n@SQ\tSN:c2\tLN:5\n"
           b"r\t83\tc1\t16385\t7\t2S3M1D2M\tc2\t3\t-9\tacgtRYn.=\tIIIIIIII!\tNM:i:255\tMD:Z:3^A2\tCB:Z:AC-GT\n"
           b"q\t0\tc2\t1\t0\t*\t*\t0\t0\tAC\t!~\tNM:i:256\tMD:Z:0\n"
           b"p\t0\tc1\t1\t0\t1M\t=\t1\t0\tA\t5\tNM:i:65536\tMD:Z:1\n")
    header, records = bm.encode(sam)
    hl = sam.index(b"r\t83")
    assert header == (b"BAM\1" + struct.pack("<I", hl) + sam[:hl] + struct.pack("<I", 2) + struct.pack("<I", 3) + b"c1\0" + struct.pack("<I", 100000) +
                      struct.pack("<I", 3) + b"c2\0" + struct.pack("<I", 5))
    first = records[:4 + struct.unpack_from("<I", records, 0)[0]]
    assert first[4:36] == struct.pack("<iiBBHHHIiii", 0, 16384, 2, 7, 4682, 4, 83, 9, 1, 2, -9)
    assert first[36:38] == b"r\0" and first[38:54] == struct.pack("<4I", 2 << 4 | 4, 3 << 4, 1 << 4 | 2, 2 << 4)
    assert first[54:59] == bytes([0x12, 0x48, 0x5a, 0xff, 0x00])
    assert first[59:68] == bytes([40] * 8 + [0])
    assert first[68:] == b"NMC\xffMDZ3^A2\0CBZAC-GT\0"
    assert b"NMS\x00\x01MDZ0\0" in records and b"NMI\x00\x00\x01\x00MDZ1\0" in records
    assert bm.decode(header + records) == bm.normalise(sam) and b"\tACGTRYNN=\t" in bm.decode(header + records)


def _smallest_bin(beg, end):
    """by the definition: the levels' windows are 2^14, 2^17, 2^20, 2^23, 2^26 and 2^29 bases, their first bins 4681, 585, 73, 9, 1, 0"""
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1), (29, 0)):
        k = beg >> shift
        if k << shift <= beg and end <= (k + 1) << shift:
            return first + k
    raise AssertionError("beyond 2^29")


def test_reg2bin_is_the_smallest_containing_bin():
    seen = set()
    for shift in (14, 17, 20, 23, 26):
        for mult in (1, 2, 3, 7):
            edge = mult << shift
            if edge >= 1 << 29:
                continue
            for beg in (edge - 2, edge - 1, edge, edge + 1):
                for length in (1, 2, 100, (1 << shift) - 1, 1 << shift, (1 << shift) + 1):
                    end = beg + length
                    if end <= 1 << 29:
                        assert bm.reg2bin(beg, end) == _smallest_bin(beg, end), (beg, end)
                        seen.add(bm.reg2bin(beg, end))
    for beg, end in ((0, 1), (0, 16384), (0, 16385), (16383, 16384), (16383, 16385), (16384, 16385), (131071, 131072), (131071, 131073),
                     ((1 << 26) - 1, 1 << 26), ((1 << 26) - 1, (1 << 26) + 1), (0, 1 << 29), ((1 << 29) - 1, 1 << 29)):
        assert bm.reg2bin(beg, end) == _smallest_bin(beg, end), (beg, end)
    assert bm.reg2bin(0, 1) == 4681 and bm.reg2bin(16383, 16385) == 585 and bm.reg2bin(0, 1 << 29) == 0
    assert {0, 1, 9, 73, 585, 4681} <= seen | {bm.reg2bin(0, 1 << 29), bm.reg2bin(0, 1 << 26), bm.reg2bin(0, 1 << 23), bm.reg2bin(0, 1 << 20),
                                              bm.reg2bin(0, 1 << 17)}
