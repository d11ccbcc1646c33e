"""The class functions of chromap_amd/csrc/cm_classes.h (which list id a list length belongs to), through the host build, against
the Python model of tests/class_ladder.py -- at B - 1, B and B + 1 of every boundary of the size-class table and around the lengths
below which a list stays with its lane.  The two are written independently: the model from the table's prose, for the GPU test."""
import ctypes as C

import pytest

import class_ladder as cl
import hostemu_lib as hl
from test_hostemu_classes import KERNEL_CLASSES, classes, lane_cap

NONE = 32                     # CM_L_NONE
S4C_PBIG = cl.PF_P[-1][0]     # the pair filter's largest class as an MI355X grants it
HIT, RESCUE, PF, S5, S6A, S6C = range(6)
BOUNDARIES = sorted(set(cl.HIT_B[50]) | set(cl.HIT_B[100]) | set(cl.CAND_B) | set(cl.NBEST_B) | set(cl.RESCUE_B))
LENGTHS = sorted({B + d for B in BOUNDARIES for d in (-1, 0, 1)} | {cl.RS_COOP_MIN, cl.RS_COOP_MIN + 1, cl.COOP_MIN, cl.COOP_MIN + 1})


def class_of(which, a, b=0, max_read_len=50, n_seq=24, goff=True, heavy_wave_max=0):
    f = hl.lib().hostemu_class_of
    f.restype = C.c_uint32
    f.argtypes = [C.POINTER(C.c_int), C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.c_uint32,
                  C.c_int, C.c_uint32, C.c_uint32]
    opts = (C.c_int * 5)(heavy_wave_max, 0, 0, 0, 0)
    return f(opts, max_read_len, lane_cap(max_read_len), n_seq, int(goff), (C.c_uint32 * 4)(*KERNEL_CLASSES), 8192, S4C_PBIG, cl.SLAB_CAP, which, a, b)


def _id(lid):
    return NONE if lid is None else lid


@pytest.mark.parametrize("goff", [True, False], ids=["key32", "key64"])
@pytest.mark.parametrize("max_read_len", [50, 100])
def test_every_boundary_at_default_classes(max_read_len, goff):
    kw = dict(max_read_len=max_read_len, goff=goff)
    cls = classes(**kw)
    assert cls["hv_big"] == (7040 if goff else 8192) and cls["hv_mid"] == (64 if max_read_len == 50 else 96)
    for a in LENGTHS:
        assert class_of(HIT, a, **kw) == _id(cl._hit_class(a, cls)), ("hit lists", a)
        assert class_of(RESCUE, a, **kw) == _id(cl._rescue_class(a, cls)), ("rescue lists", a)
        assert class_of(PF, a, **kw) == _id(cl._pf_class(a)), ("pair filter", a)
        # verification: the sum of a read's two lists decides whether a group works, the longer one which
        for p_, n_ in ((a, 0), (0, a), (a, 3), (a // 2, a - a // 2), (a - 1, 1)):
            assert class_of(S5, p_, n_, **kw) == _id(cl._s5_class(p_, n_)), ("verification", p_, n_)
        # pairing: the pair's longest list decides whether a group works, the longer list of read 2 which
        for big2 in (a, min(a, 7), min(a, cl.S6_P[0][0] + 1)):
            q = cl._s6_class(a, big2)
            assert class_of(S6A, a, big2, **kw) == (NONE if q is None else cl.S6A_LISTS[q]), ("pairing, S6a", a, big2)
            assert class_of(S6C, a, big2, **kw) == (NONE if q is None else cl.S6C_LISTS[q]), ("pairing, S6c", a, big2)


def test_lengths_that_stay_with_a_lane():
    """48 and 49 (the rescue lists: 32 and 33) on either side of every ladder's *_COOP_MIN"""
    assert (cl.COOP_MIN, cl.RS_COOP_MIN) == (48, 32)
    assert class_of(RESCUE, 32) == NONE and class_of(RESCUE, 33) == cl.RS_WAVE
    assert class_of(PF, 48) == NONE and class_of(PF, 49) == cl.PF_WAVE
    assert class_of(S5, 48, 0) == NONE and class_of(S5, 24, 24) == NONE and class_of(S5, 49, 0) == cl.S5_SMALL and class_of(S5, 24, 25) == cl.S5_SMALL
    assert class_of(S6A, 48, 48) == NONE and class_of(S6A, 49, 49) == cl.S6A_SMALL and class_of(S6A, 49, 0) == cl.S6A_SMALL
    assert class_of(S6C, 48, 48) == NONE and class_of(S6C, 49, 49) == cl.S6C_SMALL
    # the hit lists have no such constant: a lane keeps what its slots hold (16 for reads of 50 bases)
    assert class_of(HIT, 16) == NONE and class_of(HIT, 17) == cl.HIT_G16 and class_of(HIT, 48) == class_of(HIT, 49) == cl.HIT_G16


@pytest.mark.parametrize("max_read_len", [50, 100])
def test_one_lane_only(max_read_len):
    """heavy_wave_max = -1: no class at all -- every hit list beyond the lane's slots goes to list CM_L_HIT_SLAB, whose reads the host
    then gives to the one-lane kernel"""
    kw = dict(max_read_len=max_read_len, heavy_wave_max=-1)
    cls = classes(**kw)
    for a in LENGTHS:
        want = NONE if a <= cls["s3b_cap"] else cl.HIT_SLAB
        assert class_of(HIT, a, **kw) == want == _id(cl._hit_class(a, cls)), a
