"""Loads tests/hostemu/libhostemu_bai.so (tests/hostemu/hostemu_bai.cpp: the per-record and per-chunk functions and the serialiser of
chromap_amd/csrc/cm_bai.h, the device's BAM indexer, run by the host), building it when it is missing or older than its sources;
builds the stand-alone sanitizer program of the same function (tests/hostemu/bai_san_main.cpp) and writes its case files.  Test
infrastructure only."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "hostemu")
_SRCS = [os.path.join(HERE, "hostemu_bai.cpp")] + [os.path.join(ROOT, "chromap_amd", "csrc", f) for f in ("cm_bai.h", "cm_bam.h", "cm_tabix.h", "cm_types.h")]
_FLAGS = ["-std=c++17", "-g", "-fno-strict-aliasing", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas"]
_L = None


class Refused(ValueError):
    def __init__(self, cause, record):
        ValueError.__init__(self, "cause %d at record %d" % (cause, record))
        self.cause, self.record = cause, record


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
        _L = C.CDLL(_build(os.path.join(HERE, "libhostemu_bai.so"), _SRCS[0], ["-O2", "-fPIC", "-shared"]))
        _L.hostemu_bai.restype = C.c_long
        _L.hostemu_bai.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int,
                                   C.POINTER(C.c_uint64)]
    return _L


def index(data, starts, n_ref, sizes, base=0, mode=0):
    """the .bai bytes for the records `data`, record i at starts[i], whose 0xff00-byte slices became blocks of the given sizes.  mode 0:
    record by record; 1 / 2: waves of 64 lanes in ascending / descending order; 3: blocks of 256.  Refused (cause, 1-based record) for
    records that cannot be indexed"""
    n = len(data)
    src = np.frombuffer(data, np.uint8).copy() if n else np.zeros(1, np.uint8)
    st = np.asarray(starts, np.uint64)
    sz = np.asarray(list(sizes) or [0], np.uint32)
    cap = 1 << 16
    while True:
        guard = 64
        out = np.full(cap + 2 * guard, 0x5A, np.uint8)
        word = C.c_uint64(0)
        got = lib().hostemu_bai(src.ctypes.data, n, st.ctypes.data, len(st) - 1, n_ref, sz.ctypes.data, len(sizes), base, out.ctypes.data + guard, cap, mode, C.byref(word))
        assert (out[:guard] == 0x5A).all() and (out[guard + cap:] == 0x5A).all()
        if got == -1:
            cap *= 8
            continue
        if got == -2:
            raise Refused(int(word.value & 7), int(word.value >> 3) + 1)
        assert got >= 0, "hostemu_bai failed: %d" % got
        return bytes(out[guard:guard + got])


def sanitizer_program():
    """path of the stand-alone program, built with AddressSanitizer and UndefinedBehaviorSanitizer (never loaded into python)"""
    return _build(os.path.join(HERE, "bai_san"), os.path.join(HERE, "bai_san_main.cpp"), ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])


def write_case(path, data, starts, n_ref, sizes, base, want):
    """a case file of the stand-alone program"""
    with open(path, "wb") as f:
        f.write(struct.pack("<6Q", len(data), len(starts) - 1, n_ref, len(sizes), base, len(want)))
        f.write(np.asarray(starts, np.uint64).tobytes() + np.asarray(sizes, np.uint32).tobytes() + data + want)
