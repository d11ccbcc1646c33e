"""Loads tests/hostemu/libhostemu_pack_once.so (tests/hostemu/hostemu_pack_once.cpp: the stage functions of the front end's planes
route, chromap_amd/csrc/cm_stages.h, against the functions that define their results), building it when it is missing or older than
its sources; builds the stand-alone sanitizer program of the same sweeps (tests/hostemu/pack_once_san_main.cpp).  Test infrastructure
only."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "hostemu")
_HDRS = [os.path.join(ROOT, "chromap_amd", "csrc", f) for f in ("cm_stages.h", "cm_types.h", "cm_mapq_tables.h")]
_FLAGS = ["-std=c++17", "-g", "-ffp-contract=off", "-fno-strict-aliasing", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas"]
_L = None


def _build(out, srcs, flags):
    def stale():
        return not os.path.exists(out) or any(os.path.getmtime(s) > os.path.getmtime(out) for s in srcs + _HDRS)
    if stale():
        import fcntl
        with open(out + ".lock", "w") as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            if stale():
                tmp = "%s.%d.tmp" % (out, os.getpid())
                subprocess.check_call(["g++"] + _FLAGS + flags + ["-o", tmp, srcs[0]])
                os.replace(tmp, out)
    return out


def lib():
    global _L
    if _L is None:
        so = _build(os.path.join(HERE, "libhostemu_pack_once.so"), [os.path.join(HERE, "hostemu_pack_once.cpp")], ["-O2", "-fPIC", "-shared"])
        _L = C.CDLL(so)
        _L.hostemu_po_planes_check.restype = C.c_long
        _L.hostemu_po_planes_check.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        _L.hostemu_po_trim.restype = C.c_int
        _L.hostemu_po_trim.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
        _L.hostemu_po_minimizers.restype = C.c_int
        _L.hostemu_po_minimizers.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32]
    return _L


def sanitizer_program():
    """path of the stand-alone program, built with AddressSanitizer and UndefinedBehaviorSanitizer (never loaded into python)"""
    return _build(os.path.join(HERE, "pack_once_san"),
                  [os.path.join(HERE, "pack_once_san_main.cpp"), os.path.join(HERE, "hostemu_pack_once.cpp")],
                  ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
