"""Loads tests/hostemu/libhostemu_s6_planes.so (tests/hostemu/hostemu_s6_planes.cpp: S6's mismatch count on bit planes,
chromap_amd/csrc/cm_stages.h, against the byte count), building it when it is missing or older than its sources; builds the stand-alone
sanitizer program of the same cases (tests/hostemu/s6_planes_san_main.cpp).  Test infrastructure only."""
import ctypes as C
import os

from hostemu_pack_once_lib import HERE, _build

_L = None


def lib():
    global _L
    if _L is None:
        so = _build(os.path.join(HERE, "libhostemu_s6_planes.so"), [os.path.join(HERE, "hostemu_s6_planes.cpp")], ["-O2", "-fPIC", "-shared"])
        _L = C.CDLL(so)
        _L.hostemu_s6p_case.restype = C.c_int
        _L.hostemu_s6p_case.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint64, C.POINTER(C.c_int32)]
        _L.hostemu_s6p_dispatch.restype = C.c_int
        _L.hostemu_s6p_dispatch.argtypes = [C.c_int, C.c_int, C.c_uint64, C.POINTER(C.c_uint32)]
        _L.hostemu_s6p_sweep.restype = C.c_long
        _L.hostemu_s6p_sweep.argtypes = [C.c_uint64, C.POINTER(C.c_int32)]
    return _L


def sanitizer_program():
    """path of the stand-alone program, built with AddressSanitizer and UndefinedBehaviorSanitizer (never loaded into python)"""
    return _build(os.path.join(HERE, "s6_planes_san"),
                  [os.path.join(HERE, "s6_planes_san_main.cpp"), os.path.join(HERE, "hostemu_s6_planes.cpp")],
                  ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
