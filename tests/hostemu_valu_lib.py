"""Loads tests/hostemu/libhostemu_valu.so (tests/hostemu/hostemu_valu.cpp: cm_s3b_short and cm_pack_read_planes_w of
chromap_amd/csrc/cm_stages.h against the functions that define their results), building it when it is missing or older than its
sources.  Test infrastructure only."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_L = None


def lib():
    global _L
    if _L is None:
        so = os.path.join(ROOT, "tests", "hostemu", "libhostemu_valu.so")
        srcs = [os.path.join(ROOT, "tests", "hostemu", "hostemu_valu.cpp")] + \
               [os.path.join(ROOT, "chromap_amd", "csrc", f) for f in ("cm_stages.h", "cm_types.h", "cm_mapq_tables.h")]
        def stale():
            return not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs)
        if stale():
            import fcntl
            with open(so + ".lock", "w") as lock:
                fcntl.flock(lock, fcntl.LOCK_EX)
                if stale():
                    tmp = "%s.%d.tmp" % (so, os.getpid())
                    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-fPIC", "-shared", "-ffp-contract=off", "-fno-strict-aliasing",
                                           "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-o", tmp, srcs[0]])
                    os.replace(tmp, so)
        _L = C.CDLL(so)
        _L.hostemu_s3b_short_check.restype = C.c_long
        _L.hostemu_s3b_short_check.argtypes = [C.c_uint32] + [C.c_void_p] * 5 + [C.c_uint32] + [C.c_int] * 6 + [C.c_void_p] * 3 + [C.POINTER(C.c_long)]
        _L.hostemu_pack_planes_check.restype = C.c_long
        _L.hostemu_pack_planes_check.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    return _L
