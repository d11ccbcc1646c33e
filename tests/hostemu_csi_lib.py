"""Loads tests/hostemu/libhostemu_csi.so (tests/hostemu/hostemu_csi.cpp: the stage functions of chromap_amd/csrc/cm_tabix.h and
cm_bai.h with a CSI's depth, the loffset function and the CSI serialiser, run by the host), building it when it is missing or older
than its sources; builds the stand-alone sanitizer program of the same functions (tests/hostemu/csi_san_main.cpp) and writes its
case files.  Test infrastructure only."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "hostemu")
_SRCS = [os.path.join(HERE, f) for f in ("hostemu_csi.cpp", "hostemu_bai.cpp")] + [os.path.join(ROOT, "chromap_amd", "csrc", f)
                                                                                 for f in ("cm_bai.h", "cm_bam.h", "cm_tabix.h", "cm_types.h")]
_FLAGS = ["-std=c++17", "-g", "-fno-strict-aliasing", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas"]
_L = None


class Refused(ValueError):
    def __init__(self, cause, item):
        ValueError.__init__(self, "cause %d at record or line %d" % (cause, item))
        self.cause, self.item = cause, item


def _build(out, main, flags):
    srcs = [main] + _SRCS

    def stale():
        return not os.path.exists(out) or any(os.path.getmtime(s) > os.path.getmtime(out) for s in srcs)
    if stale():
        import fcntl
        with open(out + ".lock", "w") as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            if stale():
                tmp = "%s.%d.tmp" % (out, os.getpid())
                subprocess.check_call(["g++"] + _FLAGS + flags + ["-o", tmp, main])
                os.replace(tmp, out)
    return out


def lib():
    global _L
    if _L is None:
        _L = C.CDLL(_build(os.path.join(HERE, "libhostemu_csi.so"), _SRCS[0], ["-O2", "-fPIC", "-shared"]))
        _L.hostemu_csi_bam.restype = C.c_long
        _L.hostemu_csi_bam.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64,
                                       C.c_int, C.POINTER(C.c_uint64)]
        _L.hostemu_csi_bed.restype = C.c_long
        _L.hostemu_csi_bed.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.c_int, C.POINTER(C.c_uint64)]
        _L.hostemu_csi_reg2bin.restype = C.c_uint32
        _L.hostemu_csi_reg2bin.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
        _L.hostemu_csi_bin_window.restype = C.c_uint64
        _L.hostemu_csi_bin_window.argtypes = [C.c_uint32, C.c_uint32]
    return _L


def _run(call):
    cap = 1 << 16
    while True:
        guard = 64
        out = np.full(cap + 2 * guard, 0x5A, np.uint8)
        word = C.c_uint64(0)
        got = call(out.ctypes.data + guard, cap, C.byref(word))
        assert (out[:guard] == 0x5A).all() and (out[guard + cap:] == 0x5A).all()
        if got == -1:
            cap *= 8
            continue
        if got == -2:
            raise Refused(int(word.value & 7), int(word.value >> 3) + 1)
        assert got >= 0, "hostemu_csi failed: %d" % got
        return bytes(out[guard:guard + got])


def index_bam(data, starts, n_ref, sizes, depth, base=0, mode=0):
    """the CSI payload (BAM flavour) for the records `data`, record i at starts[i], whose 0xff00-byte slices became blocks of the given
    sizes.  Modes as tests/hostemu_bai_lib.py.  Refused (cause, 1-based record) for records that cannot be indexed"""
    n = len(data)
    src = np.frombuffer(data, np.uint8).copy() if n else np.zeros(1, np.uint8)
    st = np.asarray(starts, np.uint64)
    sz = np.asarray(list(sizes) or [0], np.uint32)
    return _run(lambda out, cap, word: lib().hostemu_csi_bam(src.ctypes.data, n, st.ctypes.data, len(st) - 1, n_ref, sz.ctypes.data, len(sizes), base, depth, out, cap,
                                                             mode, word))


def index_bed(text, sizes, depth, base=0, mode=0):
    """the CSI payload (tabix flavour) for the BED text whose 0xff00-byte slices became blocks of the given sizes"""
    n = len(text)
    src = np.frombuffer(text, np.uint8).copy() if n else np.zeros(1, np.uint8)
    sz = np.asarray(list(sizes) or [0], np.uint32)
    return _run(lambda out, cap, word: lib().hostemu_csi_bed(src.ctypes.data, n, sz.ctypes.data, len(sizes), base, depth, out, cap, mode, word))


def sanitizer_program():
    """path of the stand-alone program, built with AddressSanitizer and UndefinedBehaviorSanitizer (never loaded into python)"""
    return _build(os.path.join(HERE, "csi_san"), os.path.join(HERE, "csi_san_main.cpp"), ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])


def write_case(path, flavour, data, starts, n_ref, sizes, base, depth, want):
    """a case file of the stand-alone program; flavour 0: BAM records and their starts, 1: a BED text (starts ignored)"""
    with open(path, "wb") as f:
        f.write(struct.pack("<8Q", flavour, len(data), len(starts) - 1 if flavour == 0 else 0, n_ref, len(sizes), base, depth, len(want)))
        if flavour == 0:
            f.write(np.asarray(starts, np.uint64).tobytes())
        f.write(np.asarray(sizes, np.uint32).tobytes() + data + want)
