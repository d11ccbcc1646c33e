"""The size-class policy of the long-list stages (chromap_amd/csrc/cm_classes.h), through the host build: which list lengths go
to a lane, a group of 16 lanes, a wave or a block, from the options, the batch's longest read and the device's answer about the
large shared-memory allocation.  The expected values are worked out by hand from the rules."""
import ctypes as C

import pytest

import hostemu_lib as hl

KERNEL_CLASSES = (512, 1024, 2048, 4096)  # cm_s3b_heavy_classes (cm_kernels.hip)
FIELDS = ("hv_max0", "hv_max1", "hv_max2", "hv_max3", "hv_big", "rs_max3", "rs_big", "hv_mid", "hv_sub", "s3b_cap")


def lane_cap(max_read_len):  # cm_s3b_lane_cap (cm_kernels.hip): a third of the read, 16..64
    return min(64, max(16, max_read_len // 3))


def classes(max_read_len=50, n_seq=24, goff=True, hv_big_in=8192, heavy_wave_max=0, heavy_block_max=0, heavy_big_max=0,
            heavy_mid_max=0, s3b_lane_cap=0):
    L = hl.lib()
    f = L.hostemu_size_classes
    f.restype = None
    f.argtypes = [C.POINTER(C.c_int), C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_uint32), C.c_uint32,
                  C.POINTER(C.c_uint32)]
    opts = (C.c_int * 5)(heavy_wave_max, heavy_block_max, heavy_big_max, heavy_mid_max, s3b_lane_cap)
    out = (C.c_uint32 * 10)()
    f(opts, max_read_len, lane_cap(max_read_len), n_seq, int(goff), (C.c_uint32 * 4)(*KERNEL_CLASSES), hv_big_in, out)
    return dict(zip(FIELDS, out))


def row(hv_max=KERNEL_CLASSES, hv_big=7040, rs_max3=3968, rs_big=7680, hv_mid=64, hv_sub=256, s3b_cap=16):
    return dict(zip(FIELDS, tuple(hv_max) + (hv_big, rs_max3, rs_big, hv_mid, hv_sub, s3b_cap)))


NONE = dict(hv_max=(0, 0, 0, 0), hv_big=0, rs_max3=0, rs_big=0, hv_mid=0, hv_sub=0)

CASES = [
    ("defaults_len50", dict(), row()),
    ("defaults_len150", dict(max_read_len=150), row(hv_mid=96)),
    ("no_goff", dict(goff=False), row(hv_big=8192)),
    ("large_lds_refused", dict(hv_big_in=0), row(hv_big=0, rs_big=0)),
    ("one_lane_only_len50", dict(heavy_wave_max=-1), row(s3b_cap=16, **NONE)),
    ("one_lane_only_len150", dict(heavy_wave_max=-1, max_read_len=150), row(s3b_cap=50, **NONE)),
    ("forced_small_classes", dict(heavy_wave_max=18, heavy_block_max=19), row(hv_max=(18, 19, 19, 4096), hv_sub=0)),
    ("mid_and_lane_cap", dict(heavy_mid_max=256, s3b_lane_cap=4), row(hv_mid=256, s3b_cap=4)),
    # sequence ids of 2^31 and more leave no bit for the strand: no class at all; a lane's own cap stays what the read
    # length gives (k_s3b_candidates needs one)
    ("too_many_sequences", dict(n_seq=0x80000000), row(s3b_cap=16, **NONE)),
]


@pytest.mark.parametrize("name,kw,want", CASES, ids=[c[0] for c in CASES])
def test_size_classes(name, kw, want):
    assert classes(**kw) == want
