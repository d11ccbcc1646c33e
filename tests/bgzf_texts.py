"""The texts the BGZF compressor is tested on (tests/test_hostemu_deflate.py on the host emulation, tests/test_gpu_bgzf_out.py on the
device) and the checks every compressed text must pass.  Test infrastructure only."""
import gzip
import os
import struct
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SLICE = 0xff00
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
GOLDEN_TEXTS = {"sam": "s3_sam_q0.sam.gz", "bed_bc": "b1_atac_bc.bed.gz", "pairs": "h2_hic_q0.pairs.gz"}

_cache = {}


def golden_text(key):
    if key not in _cache:
        with gzip.open(os.path.join(GOLDEN, GOLDEN_TEXTS[key])) as f:
            _cache[key] = f.read()
    return _cache[key]


def _fibonacci_text():
    # Literal i fib(i + 1) times (1, 2, 3, 5, ...: the end-of-block symbol is the other 1), and nothing the match search can use: every unit is one such literal and a three-digit counter (base 60, from
    # an alphabet of its own), so no four bytes occur twice and no byte four times in a row.  Huffman's tree for the 18 Fibonacci counts is
    # a comb: the rarest literal lies 17 levels and more under the root.  No match: no distance code either.
    fib = [1, 2]
    while len(fib) < 18:
        fib.append(fib[-1] + fib[-2])
    syms = np.concatenate([np.full(c, 200 + i, np.uint8) for i, c in enumerate(fib)])
    np.random.default_rng(3).shuffle(syms)
    u = np.arange(len(syms))
    units = np.stack([syms, 48 + u // 3600, 48 + u // 60 % 60, 48 + u % 60], 1).astype(np.uint8)
    text = units.tobytes()
    assert len(text) <= SLICE
    return text


def _de_bruijn_text():
    # B(4, 4): 256 bytes over four symbols in which no four bytes occur twice -- a coded block without a match
    k, n = 4, 4
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    assert len(seq) == 256
    return bytes(b"ACGT"[x] for x in seq)


def _skewed_text(seed, n, groups):
    """n bytes drawn independently: `groups` is a list of (symbols, L) -- that many byte values of probability 2^-L each"""
    p = np.concatenate([np.full(c, 2.0 ** -L) for c, L in groups])
    return bytes(np.random.default_rng(seed).choice(len(p), n, p=p / p.sum()).astype(np.uint8))


# (1, 1, 2, 3, 5, ... literals of 2, 3, 4, ... bits: the lengths' own counts are skewed enough for a code-length tree of depth 8)
CL_DEEP_GROUPS = [(1, 2), (1, 3), (2, 4), (3, 5), (5, 6), (8, 7), (13, 8), (21, 9), (34, 10), (55, 11), (89, 12)]


def _far_match_text(distance):
    # 100 bytes that occur twice, `distance` apart, in a filler they share nothing with; the filler compresses (4 symbols), so the block is coded
    rng = np.random.default_rng(distance)
    x = bytes(rng.integers(128, 256, 100).astype(np.uint8))
    fill = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), distance - 100))
    return x + fill + x + b"ACGT" * 8


def small_texts():
    """name -> bytes: every size and shape at which the compressor takes another path (at most three slices each)"""
    if "small" not in _cache:
        rng = np.random.default_rng(7)
        line = b"chr1\t10468\t10603\tACGTACGTACGTACGT\t1\n"
        t = {}
        for n in (0, 1, 2, 3, 4):
            t["len%d" % n] = b"ACGTA"[:n]
        base = (line * (3 * SLICE // len(line) + 2))
        for name, n in (("slice-1", SLICE - 1), ("slice", SLICE), ("slice+1", SLICE + 1), ("2slices+7", 2 * SLICE + 7)):
            t[name] = base[:n]
        t["one_byte_repeated"] = b"N" * (SLICE + 300)           # matches of 258 bytes at distance 1; a last slice of 300
        t["acgt_repeated"] = b"ACGT" * 5000
        t["period3"] = b"abc" * 7000
        t["all_256_once"] = bytes(range(256))                     # no match at all, no distance code
        t["single_literal_pair"] = b"AB" * 2
        t["two_literals"] = b"Q" * 3                              # one distinct literal, no match: stored, being tiny
        t["one_literal_long"] = b"Q" * 5000                       # one distinct literal + length codes + one distance
        t["random"] = bytes(rng.integers(0, 256, SLICE + 1000).astype(np.uint8))
        t["fibonacci"] = _fibonacci_text()                        # literal code naturally deeper than 15, and no match
        t["de_bruijn"] = _de_bruijn_text()                        # no match at all in a coded block: HDIST = 1, one zero length
        t["code_length_code_deep"] = _skewed_text(1, 60000, CL_DEEP_GROUPS)  # the code-length code naturally deeper than 7
        t["match_at_32768"] = _far_match_text(32768)
        t["match_at_32769"] = _far_match_text(32769)             # one too far: must not be used
        t["last_slice_1_byte"] = base[:SLICE] + b"\n"
        t["no_match_low_entropy"] = bytes(rng.permutation(np.repeat(np.arange(48, 58, dtype=np.uint8), 40)))  # digits: coded, hardly a match
        _cache["small"] = t
    return _cache["small"]


def blocks(comp):
    """[(offset, size)] of the BGZF blocks of comp: BSIZE must walk it exactly"""
    out = []
    at = 0
    while at < len(comp):
        assert len(comp) - at >= 28, "a tail that is no block"
        assert comp[at:at + 4] == b"\x1f\x8b\x08\x04" and comp[at + 10:at + 16] == b"\x06\x00BC\x02\x00", "no BGZF header at %d" % at
        size = struct.unpack_from("<H", comp, at + 16)[0] + 1
        assert 28 <= size <= len(comp) - at
        out.append((at, size))
        at += size
    assert at == len(comp)
    return out


def check_bgzf(comp, text, inflate_block=None, own_every=1):
    """comp is `text` as one BGZF block per 0xff00-byte slice (no end-of-file block).  inflate_block(payload, n_out, crc) -> (rc, bytes):
    the project's own decoder, run on every own_every-th block and the last.  Returns the DEFLATE block type of every block (0 stored, 2 dynamic)."""
    bl = blocks(comp)
    assert len(bl) == (len(text) + SLICE - 1) // SLICE
    kinds = []
    for i, (at, size) in enumerate(bl):
        want = text[i * SLICE:(i + 1) * SLICE]
        assert size < 65536
        crc, isize = struct.unpack_from("<II", comp, at + size - 8)
        assert isize == len(want) <= SLICE
        assert crc == zlib.crc32(want)
        payload = comp[at + 18:at + size - 8]
        d = zlib.decompressobj(-15)
        got = d.decompress(payload)
        assert d.eof and d.unused_data == b"" and got == want, "block %d does not inflate to its slice" % i
        kinds.append((payload[0] >> 1) & 3)
        assert payload[0] & 1, "one final DEFLATE block per BGZF block"
        if inflate_block is not None and (i % own_every == 0 or i == len(bl) - 1):
            rc, mine = inflate_block(payload, len(want), crc)
            assert rc == 0 and mine == want, "cm_inflate.h, block %d: rc %d" % (i, rc)
    assert gzip.decompress(comp) == text
    return kinds


def zlib_level1_size(text, strategy):
    """bytes zlib needs for the same slices at level 1, with the same 26 bytes around each"""
    total = 0
    for o in range(0, len(text), SLICE):
        c = zlib.compressobj(1, zlib.DEFLATED, -15, 8, strategy)
        total += len(c.compress(text[o:o + SLICE]) + c.flush()) + 26
    return total


# ---- a DEFLATE reader of our own for the tests that look at what a block's header says
class _Bits:
    def __init__(self, data):
        self.v = int.from_bytes(data, "little")
        self.at = 0

    def take(self, n):
        x = (self.v >> self.at) & ((1 << n) - 1)
        self.at += n
        return x


def _decoder(lengths):
    """{(length, code): symbol} of the canonical code; the Kraft sum must not exceed 1"""
    table, code = {}, 0
    for l in range(1, 16):
        for sym, sl in enumerate(lengths):
            if sl == l:
                table[(l, code)] = sym
                code += 1
        code <<= 1
    return table


def _symbol(bits, table):
    code = 0
    for l in range(1, 16):
        code = (code << 1) | bits.take(1)
        if (l, code) in table:
            return table[(l, code)]
    raise AssertionError("a code word no symbol has")


def kraft(lengths, maxbits):
    """the Kraft sum of the lengths in units of 2^-maxbits: 2^maxbits for a complete code"""
    return sum(1 << (maxbits - l) for l in lengths if l)


def natural_depth(counts):
    """the longest code word Huffman's algorithm gives the counts when nothing limits it"""
    import heapq
    h = [(c, 0) for c in counts if c]
    heapq.heapify(h)
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        heapq.heappush(h, (a[0] + b[0], max(a[1], b[1]) + 1))
    return h[0][1]


def read_dynamic_block(payload):
    """A dynamic-Huffman block as this compressor writes it (lengths sent one by one).  Returns a dict: hlit, hdist, hclen, the three
    codes' lengths (cl, ll, d), the counts of the symbols the block uses (ll_cnt, d_cnt, cl_cnt) and the text (out)."""
    b = _Bits(payload)
    assert b.take(1) == 1 and b.take(2) == 2
    hlit, hdist, hclen = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
    order = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
    cl = [0] * 19
    for i in range(hclen):
        cl[order[i]] = b.take(3)
    assert cl[16] == cl[17] == cl[18] == 0
    t = _decoder(cl)
    lens = [_symbol(b, t) for _ in range(hlit + hdist)]
    cl_cnt = [lens.count(i) for i in range(19)]
    ll, d = lens[:hlit], lens[hlit:]
    tl, td = _decoder(ll), _decoder(d)
    ll_cnt, d_cnt, out = [0] * 286, [0] * 30, bytearray()
    while True:
        s = _symbol(b, tl)
        ll_cnt[s] += 1
        if s < 256:
            out.append(s)
        elif s == 256:
            break
        else:
            li = s - 257
            le = 0 if li < 8 or li == 28 else (li - 4) >> 2
            length = 258 if li == 28 else 3 + li if li < 8 else 3 + ((4 + (li & 3)) << le) + b.take(le)
            ds = _symbol(b, td)
            d_cnt[ds] += 1
            de = 0 if ds < 4 else (ds >> 1) - 1
            dist = 1 + ds if ds < 4 else 1 + ((2 + (ds & 1)) << de) + b.take(de)
            assert dist <= len(out)
            for _ in range(length):
                out.append(out[-dist])
    assert (b.at + 7) // 8 == len(payload)
    return {"hlit": hlit, "hdist": hdist, "hclen": hclen, "cl": cl, "ll": ll, "d": d, "ll_cnt": ll_cnt, "d_cnt": d_cnt, "cl_cnt": cl_cnt, "out": bytes(out)}
