"""Layout CMGPU_FASTX_FREE without a GPU: the record chain of chromap_amd/csrc/cm_fastx.h -- line classes, the walk of one record, the
resolution in tiles, the concatenating copy -- compiled for the host (tests/hostemu/hostemu_fastx.cpp, the loops in the order of the
k_fx_* launches) against a byte-level model of kseq_read (fastx_layouts.Kseq).  Built twice: with the device's tile and with a tile of
eight lines, so that records straddle every tile boundary."""
import ctypes as C
import os
import subprocess

import pytest

import fastx_layouts as fx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIBS = {}


def lib(tile=None):
    if tile not in _LIBS:
        so = os.path.join(ROOT, "tests", "hostemu", "libhostemu_fastx%s.so" % ("_t%d" % tile if tile else ""))
        srcs = [os.path.join(ROOT, "tests", "hostemu", "hostemu_fastx.cpp"), os.path.join(ROOT, "chromap_amd", "csrc", "cm_fastx.h")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
            defs = ["-DCM_FX_TILE=%du" % tile, "-DCM_FX_TILE_ROUNDS=%d" % (tile - 1).bit_length()] if tile else []
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-fPIC", "-shared", "-Wall", "-Wno-unused-function"] + defs + ["-o", so, srcs[0]])
        L = C.CDLL(so)
        L.hostemu_fastx_new.restype = C.c_void_p
        L.hostemu_fastx_free.argtypes = [C.c_void_p]
        L.hostemu_fastx_tile.restype = C.c_uint32
        L.hostemu_fastx_scan.restype = C.c_int
        L.hostemu_fastx_scan.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.hostemu_fastx_take.restype = C.c_uint64
        L.hostemu_fastx_take.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 6
        _LIBS[tile] = L
    return _LIBS[tile]


class Refused(Exception):
    def __init__(self, code):
        super().__init__("refused: %d" % code)
        self.code = code


TRUNC = 1


def parse(text, tile=None, chunk=None, limit=None, want_qual=False, fmt=None):
    """feeds `text` in chunks the way the CLI feeds the device (carry = what the take did not consume); returns names, seqs, quals"""
    L = lib(tile)
    h = L.hostemu_fastx_new()
    names, seqs, quals = [], [], []
    try:
        pos, carry = 0, b""
        chunk = chunk or max(1, len(text))
        while True:
            piece = text[pos:pos + chunk]
            pos += len(piece)
            final = pos >= len(text)
            buf = carry + piece
            n, err = C.c_uint32(0), C.c_uint32(0)
            rc = L.hostemu_fastx_scan(h, buf, len(buf), int(final), int(want_qual), C.byref(n), C.byref(err))
            if rc:
                raise Refused(rc)
            k = min(n.value, limit) if limit else n.value
            cap = len(buf) + 16
            b, q, nm = C.create_string_buffer(cap), C.create_string_buffer(cap), C.create_string_buffer(cap)
            off, noff = (C.c_uint32 * (k + 1))(), (C.c_uint32 * (k + 1))()
            hq = C.create_string_buffer(k + 1)
            nr, st, en, minus = 0, None, None, 0
            if fmt:
                nr = len(fmt[0])
                st, en, minus = (C.c_int * nr)(*fmt[0]), (C.c_int * nr)(*fmt[1]), int(fmt[2])
            used = L.hostemu_fastx_take(h, k, nr, st, en, minus, b, q, off, nm, noff, hq)
            assert used <= len(buf)
            for j in range(k):
                names.append(nm.raw[noff[j]:noff[j + 1]])
                seqs.append(b.raw[off[j]:off[j + 1]])
                quals.append(q.raw[off[j]:off[j + 1]] if hq.raw[j] == 1 else None)
            carry = buf[used:]
            if final and k == n.value:
                assert carry == b"", "a final chunk is consumed whole"
                break
    finally:
        L.hostemu_fastx_free(h)
    return names, seqs, quals


def check_equal(text, **kw):
    wn, ws, wq, trunc = fx.expected(text)
    assert not trunc
    n, s, q = parse(text, **kw)
    assert s == ws
    assert n == wn
    assert q == wq


def test_model_reads_plain_fastq_and_fasta():
    """the model itself, on texts whose records are known"""
    recs = fx.toy_records(20, 2)
    want = [(n.split()[0], s, q) for n, s, q in recs]
    for t in (fx.render(recs), fx.render(recs, width=7, plus_name=True, blanks=(0, 2)), fx.render(recs, nl=b"\r\n", width=20)):
        assert fx.Kseq(t).records() == (want, False)
    assert fx.Kseq(fx.render(recs, fasta=True, width=11)).records() == ([(n, s, None) for n, s, _ in want], False)
    assert fx.Kseq(b"@a\nACGT\n+\nIII\n").records() == ([], True)
    assert fx.Kseq(b"@a\nACGT\n+").records() == ([], True)
    assert fx.Kseq(b"@a\nAC\nGT\n+a\n@I\n+I\n@b\nA\n+\n>").records() == ([(b"a", b"ACGT", b"@I+I"), (b"b", b"A", b">")], False)


@pytest.mark.parametrize("tile", [None, 8])
def test_hand_made_layouts(tile):
    assert lib(tile).hostemu_fastx_tile() == (tile or 2048)
    for label, text in fx.hand_made():
        for chunk in (None, 4096, 1009, 97):
            if chunk and chunk < 200 and len(text) > 60000:
                continue
            try:
                check_equal(text, tile=tile, chunk=chunk)
            except AssertionError as e:
                raise AssertionError("%s, chunk %s: %s" % (label, chunk, e))
    # taken a few records at a time: bytes_consumed ends behind the last taken record
    for label, text in fx.hand_made()[:12]:
        check_equal(text, tile=tile, chunk=3000, limit=7)


def test_records_straddle_every_tile_boundary():
    """tile of eight lines: records of 2 .. 40 lines at every offset to the tile grid"""
    recs = fx.toy_records(60, 9, 30, 60)
    for lead in range(9):
        for width in (1, 3, 8, 0):
            check_equal(fx.render(recs, width=width, lead=lead, blanks=(0, 1, 0, 3)), tile=8)
            check_equal(fx.render(recs, width=width, lead=lead, fasta=True), tile=8)


def test_read_format_and_minus_strand_on_wrapped_records():
    recs = fx.toy_records(50, 11, 1, 80)
    comp = bytes.maketrans(b"ACGTacgt", b"TGCATGCA")
    for fmt in (([0], [-1], True), ([2, 30], [9, -1], False), ([5, 0], [12, 3], True), ([70], [200], False)):
        want_s, want_q = [], []
        for _, s, q in recs:
            ps, pq = b"", b""
            for a, b in zip(fmt[0], fmt[1]):
                b = len(s) - 1 if b == -1 or b >= len(s) else b
                if b >= a:
                    ps += s[a:b + 1]
                    pq += q[a:b + 1]
            if fmt[2]:
                ps = bytes(c if c in b"ACGTacgt" else ord("N") for c in ps[::-1]).upper().translate(comp)
                pq = pq[::-1]
            want_s.append(ps)
            want_q.append(pq)
        for tile in (None, 8):
            _, s, q = parse(fx.render(recs, width=7, blanks=(0, 2)), tile=tile, fmt=fmt)
            assert s == want_s and q == want_q


def test_two_thousand_texts_of_the_accepted_class():
    """zero refusals, every batch equal to the model's, for the whole text and for small chunks"""
    n_rec = 0
    for seed in range(2400):
        text = fx.accepted_text(seed)
        wn, ws, wq, trunc = fx.expected(text)
        assert not trunc, seed
        n_rec += len(ws)
        for tile, chunk in ((None, None), (8, None), (8, 61), (None, 509)):
            try:
                got = parse(text, tile=tile, chunk=chunk)
            except Refused as e:
                raise AssertionError("seed %d refused (%d), tile %s chunk %s: %r" % (seed, e.code, tile, chunk, text))
            assert got == (wn, ws, wq), "seed %d, tile %s chunk %s: %r" % (seed, tile, chunk, text)
    assert n_rec > 20000


def test_wild_texts_equal_the_model_or_are_refused():
    refused = trunc_seen = 0
    n = 4000
    for seed in range(n):
        text = fx.wild_text(seed)
        wn, ws, wq, trunc = fx.expected(text)
        trunc_seen += trunc
        for tile, chunk in ((8, None), (None, None), (8, 53)):
            try:
                got = parse(text, tile=tile, chunk=chunk)
            except Refused:
                refused += (tile, chunk) == (8, None)
                continue
            assert not trunc, "seed %d: the model says truncated quality, the chain accepted %r" % (seed, text)
            assert got == (wn, ws, wq), "seed %d, tile %s chunk %s: %r" % (seed, tile, chunk, text)
    print("wild texts: %d of %d refused; the model reports a truncated quality for %d" % (refused, n, trunc_seen))
    # (half of the damage is to qualities; what is neither a -2 of the model nor refused had to equal the model above)
    assert trunc_seen > 50 and trunc_seen <= refused < 0.7 * n


def test_refusals():
    for text, code in ((b"@a\nACGT\n+\nIII\n@b\nAC\n+\nII\n", TRUNC), (b"@a\nACGT\n+\nIIIII\n", TRUNC), (b"@a\nACGT\n+", TRUNC), (b"@a\nACGT\n+\n", TRUNC), (b"@a\nACGT\n+\nIIII\n@half\nACGT", 5), (b"@a\nACGT\n@b\nAC\n+\nII\n", 5), (b">a\nACGT\n@b\nAC\n+\nII\n", 5),
                       (b"junk\n@a\nAC\n+\nII\n", 2), (b"@a\nAC\n+\nII\nxx\n", 2), (b"@a\n\r\nAC\n+\nII\n", 3), (b"@a\nAC\n+\n\r\nII\n", 3)):
        with pytest.raises(Refused) as e:
            parse(text)
        assert e.value.code == code, text
    # a stream that needs qualities refuses records without them
    with pytest.raises(Refused) as e:
        parse(b">a\nACGT\n>b\nAC\n", want_qual=True)
    assert e.value.code == 4
    assert parse(b">a\nACGT\n>b\nAC\n") == ([b"a", b"b"], [b"ACGT", b"AC"], [None, None])
    # '@' records without a '+' line are FASTA records (kseq.h:194-206), '>' records with one are FASTQ records
    assert parse(b"@a\nACGT\n@b\nAC\n>c\nA") == ([b"a", b"b", b"c"], [b"ACGT", b"AC", b"A"], [None, None, None])
    assert parse(b">a\nACGT\n+\nIIII\n@b\nAC\n+\nII\n") == ([b"a", b"b"], [b"ACGT", b"AC"], [b"IIII", b"II"])
    # records with and without quality in one text: refused whichever chunk shows the second kind
    mixed = fx.render(fx.toy_records(30, 4), width=20) + fx.render(fx.toy_records(30, 5), fasta=True, width=20)
    for chunk in (None, 500, 97):
        with pytest.raises(Refused) as e:
            parse(mixed, chunk=chunk, tile=8)
        assert e.value.code == 5
    # a quality longer than the sequence is proven inside a non-final chunk; a shorter one is not
    with pytest.raises(Refused):
        parse(b"@a\nACGT\n+\nIIIII\n@b\nAC\n+\nII\n" * 3, chunk=20)
