"""The --barcode-translate table as the device holds it (cmgpu_barcode_translation_pack, the image cmgpu_set_barcode_translation
uploads), made and probed on the CPU: the image is read here with the layout and hash include/chromap_amd.h documents and compared
with a dict built by a parser of the same rules written in Python.  cmgpu_barcode_translate_host runs the lookup, segment and render
functions of the device writers (cm_barcode_translate.h) on the host: it is compared with a Python model of the reference's shifts
(barcode_translator.h:80-83).  No GPU."""
import ctypes as C
import random

import numpy as np
import pytest

from chromap_amd import _capi

EINVAL, ECAPACITY, EFORMAT = -1, -5, -7
HASH_MUL = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1
EMPTY = M64


def key_of(seq):
    k = 0
    for ch in seq:
        k = (k << 2) | {"A": 0, "C": 1, "G": 2, "T": 3}.get(ch.upper(), 0)
    return k & M64


def parse(text):
    """{key: to}, from_length -- the rules of the header: to<TAB or ,>from, last line of a key wins, the last line's `from` length
    is the segment length, a line without a separator is skipped"""
    table, from_len = {}, 0
    for line in text.split(b"\n"):
        seps = [i for i, c in enumerate(line) if c in b",\t"]
        if not seps:
            continue
        i = seps[0]
        frm = line[i + 1:].decode("latin-1")
        from_len = len(frm)
        table[key_of(frm)] = line[:i]
    return table, from_len


def pack(text, bucket_capacity=None, blob_capacity=None):
    """(rc, buckets array or None, blob bytes or None, n_buckets, blob_bytes, from_length)"""
    L = _capi.lib()
    nb, bb, fl = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
    rc = L.cmgpu_barcode_translation_pack(text, len(text), None, 0, None, 0, C.byref(nb), C.byref(bb), C.byref(fl))
    if rc:
        return rc, None, None, nb.value, bb.value, fl.value
    sizes = (nb.value, bb.value, fl.value)
    bc = nb.value if bucket_capacity is None else bucket_capacity
    lc = bb.value if blob_capacity is None else blob_capacity
    buckets = np.full(2 * max(bc, 1), 0x5555555555555555, np.uint64)
    blob = np.full(max(lc, 1) + 8, 0x7e, np.uint8)
    nb2, bb2, fl2 = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
    rc = L.cmgpu_barcode_translation_pack(text, len(text), buckets.ctypes.data, bc, blob.ctypes.data, lc, C.byref(nb2), C.byref(bb2), C.byref(fl2))
    assert (nb2.value, bb2.value, fl2.value) == sizes  # the sizes are reported whatever the capacities
    assert bytes(blob[max(lc, 1):]) == b"\x7e" * 8     # nothing past the capacity
    return rc, buckets, bytes(blob[:bb.value]), nb.value, bb.value, fl.value


def probe(buckets, n_buckets, blob, key):
    """the `to` string of key, or None -- the documented probe sequence; also returns the steps taken"""
    b = ((key * HASH_MUL & M64) >> 32) & (n_buckets - 1)
    for step in range(n_buckets + 1):
        k, v = int(buckets[2 * b]), int(buckets[2 * b + 1])
        if v == EMPTY:
            return None, step
        if k == key:
            off, ln = v >> 32, v & 0xffffffff
            assert off + ln <= len(blob)
            return blob[off:off + ln], step
        b = (b + 1) & (n_buckets - 1)
    raise AssertionError("the table has no empty bucket")


def check_image(text, absent=()):
    want, from_len = parse(text)
    rc, buckets, blob, nb, bb, fl = pack(text)
    assert rc == 0
    assert fl == from_len
    assert nb >= 16 and nb & (nb - 1) == 0 and nb >= 2 * len(want)  # a power of two, load factor <= 0.5
    assert nb == max(16, 1 << (2 * len(want) - 1).bit_length())
    assert bb == sum(len(v) for v in want.values()) == len(blob)
    used = [i for i in range(nb) if int(buckets[2 * i + 1]) != EMPTY]
    assert len(used) == len(want)
    assert sorted(int(buckets[2 * i]) for i in used) == sorted(want)
    max_steps = 0
    for k, to in want.items():
        got, steps = probe(buckets, nb, blob, k)
        assert got == to, (k, got, to)
        max_steps = max(max_steps, steps)
    for k in absent:
        if k not in want:
            assert probe(buckets, nb, blob, k)[0] is None
    return want, buckets, blob, nb, fl, max_steps


def test_separators_empty_to_repeats_letters_and_lines_to_skip():
    text = (b"tab_name\tACGTACGT\n"
            b"comma_name,CCCCGGGG\n"
            b"\tTTTTTTTT\n"              # empty `to`
            b"first,AAAACCCC\n"
            b"no separator here\n"       # skipped
            b"\n"                        # skipped
            b"second\tAAAACCCC\n"        # the same key again: the last line wins
            b"lower,acgtacgn\n"          # lower case; n counts as A
            b"both\t,GGGGGGGG\n"         # the FIRST separator splits: `from` is ",GGGGGGGG" (9 letters, the comma counts as A)
            b"last,GATTACAG")            # no final newline
    want, buckets, blob, nb, fl, _ = check_image(text, absent=[key_of("GGGGGGGT"), key_of("CATCATCA"), 0xffff])
    assert fl == 8
    assert want[key_of("AAAACCCC")] == b"second"
    assert want[key_of("TTTTTTTT")] == b""
    assert want[key_of("ACGTACGA")] == b"lower"
    assert want[key_of("AGGGGGGGG")] == b"both"
    assert want[key_of("GATTACAG")] == b"last"
    assert len(want) == 7


def test_acgn_lands_on_the_key_of_acga():
    want, *_ = check_image(b"x\tacgn\n")
    assert list(want) == [key_of("ACGA")] and want[key_of("ACGA")] == b"x"


def test_all_256_four_base_keys_chains_and_wrap():
    seqs = ["".join("ACGT"[(k >> s) & 3] for s in (6, 4, 2, 0)) for k in range(256)]
    text = b"".join(b"name_%03d_%s\t%s\n" % (k, b"x" * (k % 7), s.encode()) for k, s in enumerate(seqs))
    want, buckets, blob, nb, fl, max_steps = check_image(text, absent=[256, 1 << 40, M64])
    assert len(want) == 256 and nb == 512 and fl == 4
    # The hash is a multiplication by 2^64 / phi: it spreads consecutive small keys evenly, so these 256 keys all sit in their home
    # buckets (max_steps == 0 is a property of the hash, not asserted).  Chains and the wrap at the table's end are therefore made
    # with chosen keys: six 8-base keys whose home is one of the last two of 16 buckets -- inserted in increasing order they fill
    # buckets 14 / 15 and go on at 0, 1, ...
    home = lambda k: ((k * HASH_MUL & M64) >> 32) & 15
    tail = [k for k in range(1, 65536) if home(k) >= 14][:6]
    assert len(tail) == 6
    small = b"".join(b"w%d,%s\n" % (k, "".join("ACGT"[(k >> (2 * s)) & 3] for s in range(7, -1, -1)).encode()) for k in tail)
    w2, b2, blob2, nb2, fl2, steps2 = check_image(small, absent=[k for k in range(1, 65536) if home(k) >= 13][:40])
    assert nb2 == 16 and fl2 == 8 and steps2 >= 4
    used = sorted(i for i in range(16) if int(b2[2 * i + 1]) != EMPTY)
    assert used[-1] == 15 and used[0] == 0 and len(used) == 6  # the chain runs over the table's end


def test_all_ones_is_a_key_like_any_other():
    text = b"poly_t\t" + b"T" * 32 + b"\n" + b"poly_a," + b"A" * 32 + b"\n"
    want, buckets, blob, nb, fl, _ = check_image(text, absent=[1, 12345])
    assert fl == 32 and want[M64] == b"poly_t" and want[0] == b"poly_a"


def test_100000_random_16_base_keys():
    rng = random.Random(20240611)
    seqs = set()
    while len(seqs) < 100000:
        seqs.add("".join(rng.choice("ACGT") for _ in range(16)))
    lines = [b"%s%s%s" % (b"n%d" % i if i % 11 else b"", b"\t" if i & 1 else b",", s.encode()) for i, s in enumerate(sorted(seqs))]
    rng.shuffle(lines)
    text = b"\n".join(lines) + b"\n"
    absent = [rng.getrandbits(32) for _ in range(2000)]
    want, buckets, blob, nb, fl, max_steps = check_image(text, absent=absent)
    assert len(want) == 100000 and nb == 262144 and fl == 16


@pytest.mark.parametrize("text", [b"", b"\n\n", b"no separator\nnone here either\n", b"name\t\n"])
def test_no_usable_line_is_einval(text):
    # (the last: an empty `from` -- a segment length of 0 translates nothing, the reference divides by it)
    assert pack(text)[0] == EINVAL


def test_sizes_only_then_exact_capacity_then_too_small():
    text = b"".join(b"cell-%d\t%s\n" % (i, "".join("ACGT"[(i >> (2 * s)) & 3] for s in range(7, -1, -1)).encode()) for i in range(40))
    L = _capi.lib()
    nb, bb, fl = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
    assert L.cmgpu_barcode_translation_pack(text, len(text), None, 0, None, 0, C.byref(nb), C.byref(bb), C.byref(fl)) == 0
    assert (nb.value, fl.value) == (128, 8) and bb.value == sum(len(b"cell-%d" % i) for i in range(40))
    # the size outputs are optional too
    assert L.cmgpu_barcode_translation_pack(text, len(text), None, 0, None, 0, None, None, None) == 0
    rc, buckets, blob, *_ = pack(text)  # exact capacities
    assert rc == 0
    assert probe(buckets, 128, blob, 39)[0] == b"cell-39"
    for bc, lc in [(nb.value - 1, None), (None, bb.value - 1), (0, 0), (64, None)]:
        rc, _, _, nb2, bb2, fl2 = pack(text, bucket_capacity=bc, blob_capacity=lc)
        assert rc == ECAPACITY and (nb2, bb2, fl2) == (nb.value, bb.value, 8)


def model_translate(table, from_len, key, bc_len):
    """the reference's Translate (barcode_translator.h:73-100) with its shifts on 64-bit values; None: a segment is not in the table"""
    n = bc_len // from_len
    mask = M64 if from_len >= 32 else (1 << (2 * from_len)) - 1
    out = []
    for i in range(n):
        seed = (((key << (2 * i * from_len)) & M64) >> (2 * (n - 1) * from_len)) & mask
        if seed not in table:
            return None
        out.append(table[seed])
    return b"-".join(out)


def host_translate(buckets, nb, blob, fl, key, bc_len, capacity=20000):
    L = _capi.lib()
    out = C.create_string_buffer(capacity + 1)
    n = C.c_uint64(0)
    rc = L.cmgpu_barcode_translate_host(buckets.ctypes.data, nb, blob, fl, key, bc_len, out, capacity, C.byref(n))
    return rc, out.raw[:n.value] if rc == 0 else None, n.value


@pytest.mark.parametrize("from_len,bc_len", [(16, 16), (8, 16), (4, 12), (5, 16), (3, 32), (7, 30), (20, 16), (32, 32), (16, 32), (1, 32)])
def test_host_twin_of_the_device_function_follows_the_reference_shifts(from_len, bc_len):
    rng = random.Random(100 * from_len + bc_len)
    n_keys = min(200, 4 ** from_len)
    keys = rng.sample(range(4 ** from_len), n_keys) if from_len <= 10 else [rng.getrandbits(2 * from_len) for _ in range(n_keys)]
    seq = lambda k: "".join("ACGT"[(k >> (2 * (from_len - 1 - j))) & 3] for j in range(from_len))
    text = b"".join(b"%s\t%s\n" % (b"N" * (i % 13) + b"%d" % i, seq(k).encode()) for i, k in enumerate(keys))
    table, fl = parse(text)
    rc, buckets, blob, nb, _, fl2 = pack(text)
    assert rc == 0 and fl == fl2 == from_len
    hits = misses = 0
    for trial in range(400):
        n = bc_len // from_len
        rem = bc_len - n * from_len
        if trial % 4 and n:  # table entries in the low n * from_len bases, where the reference's shifts look; anything above them
            key = rng.getrandbits(2 * rem) if rem else 0
            for _ in range(n):
                key = (key << (2 * from_len)) | rng.choice(keys)
        else:
            key = rng.getrandbits(2 * bc_len)
        want = model_translate(table, from_len, key, bc_len)
        rc, got, n_out = host_translate(buckets, nb, blob, fl, key, bc_len)
        if want is None:
            assert rc == EFORMAT
            misses += 1
        else:
            assert rc == 0 and got == want
            hits += 1
            if len(want):
                assert host_translate(buckets, nb, blob, fl, key, bc_len, capacity=len(want) - 1)[0::2] == (ECAPACITY, len(want))
    if from_len > bc_len:
        assert misses == 0  # no segment: the column is empty whatever the barcode
        assert host_translate(buckets, nb, blob, fl, 12345, bc_len)[:2] == (0, b"")
    else:
        assert hits > 0


def test_an_image_without_an_empty_bucket_ends_the_search_as_a_miss():
    """the packer never fills a table, but cmgpu_barcode_translate_host takes any caller's image: the probe is bounded"""
    nb = 16
    buckets = np.zeros(2 * nb, np.uint64)
    for b in range(nb):
        buckets[2 * b], buckets[2 * b + 1] = 1000 + b, 1  # every bucket taken: {key, offset 0, length 1}
    assert host_translate(buckets, nb, b"x", 8, 1000 + 5, 8)[:2] == (0, b"x")
    assert host_translate(buckets, nb, b"x", 8, 77, 8)[0] == EFORMAT
