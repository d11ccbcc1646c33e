"""The reads' bit planes four bytes at a time (cm_pack_read_planes_w, chromap_amd/csrc/cm_stages.h: SWAR case fold, Gray decode and
letter test, the length applied once per word) against the byte-at-a-time definition (cm_pack_read_planes_any over cm_c2u), compiled
for the host (tests/hostemu/hostemu_valu.cpp): every length 1 .. 256 at every start alignment 0 .. 7, forward and reverse-complement
planes, the bytes drawn from the letters in both cases, N, and the neighbours of the letter ranges."""
import ctypes as C

import numpy as np

from hostemu_valu_lib import lib

ALPHABET = b"ACGTacgtNn@[`{\x00\xff"


def run(pool):
    pool = np.ascontiguousarray(pool, dtype=np.uint8)
    bl, ba = C.c_uint32(0), C.c_uint32(0)
    rc = lib().hostemu_pack_planes_check(pool.ctypes.data, len(pool), 256, C.byref(bl), C.byref(ba))
    assert rc >= 0, "planes differ at length %d, alignment %d (rc %d)" % (bl.value, ba.value, rc)
    return rc


def test_planes_of_every_length_and_alignment():
    rng = np.random.default_rng(20261019)
    letters = np.frombuffer(ALPHABET, np.uint8)
    # mostly letters (so that whole words are valid), every other byte of the alphabet often enough to land on every lane of a word
    p = np.array([8] * 8 + [1] * (len(letters) - 8), float)
    pool = rng.choice(letters, 1 << 16, p=p / p.sum())
    assert run(pool) >= 256 * 8


def test_planes_of_every_byte_value():
    # each of the 256 byte values on each of the eight lanes of an aligned word, between letters
    rng = np.random.default_rng(7)
    pool = rng.choice(np.frombuffer(b"ACGTacgt", np.uint8), 1 << 16)
    pool[::3] = np.arange(len(pool[::3])) % 256
    assert run(pool) >= 256 * 8
