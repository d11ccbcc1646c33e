"""Loads tests/hostemu/libhostemu_deflate.so (tests/hostemu/hostemu_deflate.cpp: cm_deflate_block of chromap_amd/csrc/cm_deflate.h, the
device's BGZF compressor, run by emulated lanes), building it when it is missing or older than its sources.  Test infrastructure only."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLICE = 0xff00
_L = None


def lib():
    global _L
    if _L is None:
        so = os.path.join(ROOT, "tests", "hostemu", "libhostemu_deflate.so")
        srcs = [os.path.join(ROOT, "tests", "hostemu", f) for f in ("hostemu_deflate.cpp", "emu_group.h")] + \
               [os.path.join(ROOT, "chromap_amd", "csrc", f) for f in ("cm_deflate.h", "cm_inflate.h", "cm_types.h")]
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
        _L.hostemu_deflate.restype = C.c_long
        _L.hostemu_deflate.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.POINTER(C.c_uint64)]
        _L.hostemu_deflate_shared_bytes.restype = C.c_uint32
        _L.hostemu_df_huff.restype = None
        _L.hostemu_df_huff.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int]
    return _L


def deflate(text, mode=0):
    """The BGZF blocks of `text` (bytes) as the device writes them.  mode 0: one lane; 1 / 2: 64 emulated lanes in ascending /
    descending order; 3: 256 lanes."""
    n = len(text)
    n_slices = (n + SLICE - 1) // SLICE
    cap = n + 64 * n_slices + 64
    guard = 64
    out = np.full(cap + 2 * guard, 0x5A, np.uint8)
    src = np.frombuffer(text, np.uint8).copy() if n else np.zeros(1, np.uint8)
    nb = C.c_uint64(0)
    got = lib().hostemu_deflate(src.ctypes.data, n, out.ctypes.data + guard, cap, mode, C.byref(nb))
    assert got >= 0, "hostemu_deflate failed: %d" % got
    assert (out[:guard] == 0x5A).all() and (out[guard + cap:] == 0x5A).all()
    assert nb.value == n_slices
    return bytes(out[guard:guard + got])


def huff_lengths(counts, maxbits, mode=0):
    """cm_df_huff: the code lengths (at most maxbits) for the symbols' counts"""
    cnt = np.asarray(counts, np.uint32).copy()
    out = np.full(len(cnt) + 16, 0x5A, np.uint8)
    lib().hostemu_df_huff(cnt.ctypes.data, len(cnt), maxbits, out.ctypes.data + 8, mode)
    assert (out[:8] == 0x5A).all() and (out[8 + len(cnt):] == 0x5A).all()
    return [int(x) for x in out[8:8 + len(cnt)]]
