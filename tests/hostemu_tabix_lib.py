"""Loads tests/hostemu/libhostemu_tabix.so (tests/hostemu/hostemu_tabix.cpp: the tile, line and chunk functions and the serialiser of
chromap_amd/csrc/cm_tabix.h, the device's tabix indexer, run by the host), building it when it is missing or older than its sources.
Test infrastructure only."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_L = None


class Refused(ValueError):
    def __init__(self, cause, line):
        ValueError.__init__(self, "cause %d at line %d" % (cause, line))
        self.cause, self.line = cause, line


CAUSES = {1: "malformed", 2: "name recurs", 3: "not sorted", 4: "beyond 2^29"}


def lib():
    global _L
    if _L is None:
        so = os.path.join(ROOT, "tests", "hostemu", "libhostemu_tabix.so")
        srcs = [os.path.join(ROOT, "tests", "hostemu", f) for f in ("hostemu_tabix.cpp", "emu_group.h")] + \
               [os.path.join(ROOT, "chromap_amd", "csrc", f) for f in ("cm_tabix.h", "cm_types.h")]
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
        _L.hostemu_tabix.restype = C.c_long
        _L.hostemu_tabix.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.POINTER(C.c_uint64)]
        _L.hostemu_tabix_reg2bin.restype = C.c_uint32
        _L.hostemu_tabix_reg2bin.argtypes = [C.c_uint32, C.c_uint32]
    return _L


def index(text, sizes, base=0, mode=0):
    """the index payload of `text` whose slices became blocks of the given sizes.  mode 0: one lane; 1 / 2: 64 emulated lanes in
    ascending / descending order (2: every loop backwards); 3: 256 lanes.  Refused (cause, 1-based line) for a text that cannot be
    indexed; ValueError("no final newline")"""
    n = len(text)
    src = np.frombuffer(text, np.uint8).copy() if n else np.zeros(1, np.uint8)
    sz = np.asarray(list(sizes) or [0], np.uint32)
    cap = 1 << 16
    while True:
        guard = 64
        out = np.full(cap + 2 * guard, 0x5A, np.uint8)
        word = C.c_uint64(0)
        got = lib().hostemu_tabix(src.ctypes.data, n, sz.ctypes.data, len(sizes), base, out.ctypes.data + guard, cap, mode, C.byref(word))
        assert (out[:guard] == 0x5A).all() and (out[guard + cap:] == 0x5A).all()
        if got == -1:
            cap *= 8
            continue
        if got == -2:
            raise Refused(int(word.value & 7), int(word.value >> 3) + 1)
        if got == -3:
            raise ValueError("no final newline")
        assert got >= 0, "hostemu_tabix failed: %d" % got
        return bytes(out[guard:guard + got])


def reg2bin(beg, end):
    return int(lib().hostemu_tabix_reg2bin(beg, end))
