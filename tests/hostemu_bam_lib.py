"""Loads tests/hostemu/libhostemu_bam.so (tests/hostemu/hostemu_bam.cpp: the record size function and the group encoder of
chromap_amd/csrc/cm_bam.h, the device's BAM writer, run by the host under emulated lanes), building it when it is missing or older
than its sources; and puts SAM lines back into the layout of the device's stores.  Test infrastructure only."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_L = None
GUARD = 256


def lib():
    global _L
    if _L is None:
        so = os.path.join(ROOT, "tests", "hostemu", "libhostemu_bam.so")
        srcs = [os.path.join(ROOT, "tests", "hostemu", f) for f in ("hostemu_bam.cpp", "emu_group.h")] + \
               [os.path.join(ROOT, "chromap_amd", "csrc", f) for f in ("cm_bam.h", "cm_types.h")]
        def stale():
            return not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs)
        if stale():
            import fcntl
            with open(so + ".lock", "w") as lock:
                fcntl.flock(lock, fcntl.LOCK_EX)
                if stale():
                    tmp = "%s.%d.tmp" % (so, os.getpid())
                    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-fPIC", "-shared", "-fno-strict-aliasing",
                                           "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-o", tmp, srcs[0]])
                    os.replace(tmp, so)
        _L = C.CDLL(so)
        _L.hostemu_bam_encode.restype = C.c_long
        _L.hostemu_bam_encode.argtypes = [C.c_int, C.c_int, C.c_uint64] + [C.c_void_p] * 11 + [C.c_int, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64,
                                                                                              C.c_void_p, C.POINTER(C.c_uint64)]
        _L.hostemu_bam_reg2bin.restype = C.c_uint32
        _L.hostemu_bam_reg2bin.argtypes = [C.c_uint32, C.c_uint32]
        _L.hostemu_bam_code.restype = C.c_uint32
        _L.hostemu_bam_code.argtypes = [C.c_uint32, C.c_int]
        _L.hostemu_bam_sub33.restype = C.c_uint32
        _L.hostemu_bam_sub33.argtypes = [C.c_uint32]
    return _L


_COMP = bytes.maketrans(b"ACGTacgt", b"TGCATGCA")


def revcomp(seq):
    """sp_comp of cm_sam_post.hip, reversed: anything but ACGT (either case) gives N"""
    return bytes((_COMP[c] if chr(c) in "ACGTacgt" else ord("N")) for c in seq[::-1])


class Store:
    """records in the layout of the device's stores: twelve words per record, CIGAR words, MD bytes, names, reads as they were read"""

    def __init__(self, cb_len=0):
        self.rec, self.cigar, self.cigar_off, self.md, self.md_off = [], [], [0], bytearray(), [0]
        self.names, self.name_off, self.bases, self.quals, self.read_off, self.bc = bytearray(), [0], bytearray(), bytearray(), [0], []
        self.cb_len = cb_len

    def add(self, rid, pos, mrid, mpos, tlen, flag, mapq, nm, cigar_words, md, name, bases, quals, strand, trim_len, barcode=None):
        assert len(bases) == len(quals) >= trim_len
        self.rec.append([rid, pos, mpos, nm, mrid & 0xffffffff, tlen & 0xffffffff, flag, len(cigar_words), len(md), mapq, strand, trim_len])
        self.cigar += cigar_words
        self.cigar_off.append(len(self.cigar))
        self.md += md
        self.md_off.append(len(self.md))
        self.names += name
        self.name_off.append(len(self.names))
        self.bases += bases
        self.quals += quals
        self.read_off.append(len(self.bases))
        key = 0
        if self.cb_len:
            assert len(barcode) == self.cb_len
            for ch in barcode.decode():
                key = key << 2 | "ACGT".index(ch)
        self.bc.append(key)

    def __len__(self):
        return len(self.rec)


def store_from_sam(sam_text):
    """the records of a SAM text back in the stores' layout: the read of a line with flag & 16 returns to the orientation it was read in"""
    refs, lines = [], []
    for ln in sam_text.split(b"\n"):
        if ln.startswith(b"@SQ"):
            refs.append(dict(x.split(b":", 1) for x in ln.split(b"\t")[1:])[b"SN"])
        elif ln and not ln.startswith(b"@"):
            lines.append(ln.split(b"\t"))
    rid_of = {nm: i for i, nm in enumerate(refs)}
    cb = [f[5:] for f in lines[0][11:] if f.startswith(b"CB:Z:")] if lines else []
    st = Store(len(cb[0]) if cb else 0)
    for c in lines:
        tags = {f[:2]: f[5:] for f in c[11:]}
        words, num = [], 0
        for ch in c[5].decode():
            if ch.isdigit():
                num = num * 10 + int(ch)
            elif ch != "*":
                words.append(num << 4 | "MIDNSHP=X".index(ch))
                num = 0
        rid = rid_of[c[2]]
        mrid = -1 if c[6] == b"*" else rid if c[6] == b"=" else rid_of[c[6]]
        minus = int(c[1]) & 16
        st.add(rid, int(c[3]) - 1, mrid, int(c[7]) - 1 if mrid >= 0 else 0, int(c[8]), int(c[1]), int(c[4]), int(tags[b"NM"]), words, tags[b"MD"], c[0],
               revcomp(c[9]) if minus else c[9], c[10][::-1] if minus else c[10], 0 if minus else 1, len(c[9]), tags.get(b"CB"))
    return st


def encode(st, G, reverse=False, start=0, fill=0x5A):
    """(bytes written from `start` on, the records' offsets, refused records); the bytes around the output are checked for `fill`"""
    n = len(st)
    rec = np.asarray(st.rec, np.uint32).reshape(-1, 12) if n else np.zeros((1, 12), np.uint32)
    arr = lambda x, t: np.asarray(list(x) or [0], t)
    cigar, cigar_off, md_off = arr(st.cigar, np.uint32), arr(st.cigar_off, np.uint64), arr(st.md_off, np.uint64)
    name_off, read_off, bc = arr(st.name_off, np.uint64), arr(st.read_off, np.uint64), arr(st.bc, np.uint64)
    buf = lambda b: np.frombuffer(bytes(b) or b"\0", np.uint8).copy()
    md, names, bases, quals = buf(st.md), buf(st.names), buf(st.bases), buf(st.quals)
    cap = start + 64 + sum(64 + 4 * r[7] + r[8] + 2 * r[11] for r in st.rec) + len(st.names) + n * st.cb_len  # (room to spare)
    room = np.full(GUARD + cap + GUARD, fill, np.uint8)
    base = room.ctypes.data + GUARD
    assert base % 4 == 0
    off = np.zeros(n + 1, np.uint64)
    refused = C.c_uint64(0)
    p = lambda a: a.ctypes.data
    end = lib().hostemu_bam_encode(G, int(reverse), n, p(rec), p(cigar), p(cigar_off), p(md), p(md_off), p(names), p(name_off), p(bases), p(quals),
                                   p(read_off), p(bc), int(st.cb_len > 0), st.cb_len, base, start, cap, p(off), C.byref(refused))
    assert end >= 0, "hostemu_bam_encode failed: %d" % end
    assert (room[:GUARD + start] == fill).all() and (room[GUARD + end:] == fill).all(), "bytes outside the records were written"
    return bytes(room[GUARD + start:GUARD + end]), [int(x) for x in off], int(refused.value)
