"""Loads tests/hostemu/libhostemu_valu.so (tests/hostemu/hostemu_valu.cpp: cm_s3b_short and cm_pack_read_planes_w of
chromap_amd/csrc/cm_stages.h against the functions that define their results, and the MAPQ functions on plain arguments), building it
when it is missing or older than its sources; builds the stand-alone sanitizer program of the MAPQ cases
(tests/hostemu/mapq_san_main.cpp).  Test infrastructure only."""
import ctypes as C
import os

from hostemu_pack_once_lib import HERE, _build

_L = None


def lib():
    global _L
    if _L is None:
        so = _build(os.path.join(HERE, "libhostemu_valu.so"), [os.path.join(HERE, "hostemu_valu.cpp")], ["-O2", "-fPIC", "-shared"])
        _L = C.CDLL(so)
        _L.hostemu_s3b_short_check.restype = C.c_long
        _L.hostemu_s3b_short_check.argtypes = [C.c_uint32] + [C.c_void_p] * 5 + [C.c_uint32] + [C.c_int] * 6 + [C.c_void_p] * 3 + [C.POINTER(C.c_long)]
        _L.hostemu_pack_planes_check.restype = C.c_long
        _L.hostemu_pack_planes_check.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        _L.hostemu_mapq_batch.restype = C.c_int
        _L.hostemu_mapq_batch.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                          C.POINTER(C.c_uint32)]
    return _L


def mapq_batch(kind, e, reads, pairs):
    """the product's MAPQ stage functions on the host: reads int32 [9, 2 n], pairs int32 [6, n] -> uint8 [n]"""
    import numpy as np
    reads = np.ascontiguousarray(reads, dtype=np.int32)
    pairs = np.ascontiguousarray(pairs, dtype=np.int32)
    n = pairs.shape[1]
    assert reads.shape == (9, 2 * n) and pairs.shape == (6, n)
    out = np.full(n, 0xEE, np.uint8)
    assert lib().hostemu_mapq_batch(kind, e, n, reads.ctypes.data, pairs.ctypes.data, out.ctypes.data, None, None, 0, None) == 0
    return out


def mapq_tables():
    """(len_coef float64 [65536], nsec_break uint32 [n_break]) as cm_mapq_tables.h builds them"""
    import numpy as np
    coef = np.zeros(65536, np.float64)
    brk = np.zeros(256, np.uint32)
    nb = C.c_uint32(0)
    assert lib().hostemu_mapq_batch(0, 0, 0, None, None, None, coef.ctypes.data, brk.ctypes.data, len(brk), C.byref(nb)) == 0
    return coef, brk[:nb.value]


def mapq_sanitizer_program():
    """path of the stand-alone program, built with AddressSanitizer and UndefinedBehaviorSanitizer including the float-cast check
    (never loaded into python)"""
    return _build(os.path.join(HERE, "mapq_san"), [os.path.join(HERE, "mapq_san_main.cpp"), os.path.join(HERE, "hostemu_valu.cpp")],
                  ["-O1", "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=undefined,float-cast-overflow"])
