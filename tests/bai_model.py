"""The BAM index (.bai) in plain Python, written from the SAM specification (section 5.2: bins of the UCSC scheme, chunks of virtual
offsets, the 16 kb linear index, the pseudo-bin 37450) and from the rules the device's builder states for what the specification
leaves open (chromap_amd/csrc/cm_bai.h): raw chunks are maximal runs of records with one (reference, bin) in file order, a chunk joins
the one before it in its bin when it begins in the block in which that one ends or an earlier one, empty windows are filled from
the right, a reference without records has neither bins nor windows, bins are not folded into their parents.  Also a reader of the
format and a region query through it, with the brute-force query it must agree with.  Test infrastructure only."""
import struct
import zlib

import bam_model as bm
import bgzf_texts as bt

MALFORMED, NOREF, UNSORTED, RANGE = 1, 2, 3, 4
CAUSES = {MALFORMED: "malformed", NOREF: "no reference", UNSORTED: "not sorted", RANGE: "beyond 2^29"}
MAX_END = 1 << 29
PSEUDO_BIN = 37450


class NotIndexable(ValueError):
    def __init__(self, cause, record):
        ValueError.__init__(self, "record %d: %s" % (record, CAUSES[cause]))
        self.cause, self.record = cause, record


def bgzf_blocks_of(data, level=1):
    """`data` as BGZF blocks of at most 0xff00 bytes each (no end-of-file block): what a host writes in front of the device's blocks"""
    out = []
    for at in range(0, len(data), bt.SLICE):
        piece = data[at:at + bt.SLICE]
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        body = c.compress(piece) + c.flush()
        size = 18 + len(body) + 8
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", size - 1) + body + struct.pack("<II", zlib.crc32(piece), len(piece)))
    return b"".join(out)


def bam_header(n_ref, length=MAX_END):
    """an uncompressed BAM header with n_ref references ref0, ref1, ..."""
    return bm.encode(b"".join(b"@SQ\tSN:ref%d\tLN:%d\n" % (i, length) for i in range(n_ref)))[0]


class File:
    """a whole BAM file taken apart: the inflated bytes, where each block's bytes begin in them, the header's end"""

    def __init__(self, raw):
        self.block_at, self.u_at = [], []   # file offset and first inflated byte of every block, the end-of-file block(s) included
        parts, u = [], 0
        for at, size in bt.blocks(raw):
            d = zlib.decompressobj(-15)
            piece = d.decompress(raw[at + 18:at + size - 8])
            assert d.eof and struct.unpack_from("<I", raw, at + size - 4)[0] == len(piece)
            self.block_at.append(at)
            self.u_at.append(u)
            parts.append(piece)
            u += len(piece)
        self.block_at.append(len(raw))
        self.u_at.append(u)
        self.data = b"".join(parts)
        self.lens = [len(p) for p in parts] + [0]
        b = self.data
        assert b[:4] == b"BAM\1", "no BAM magic"
        at = 8 + struct.unpack_from("<I", b, 4)[0]
        (self.n_ref,) = struct.unpack_from("<I", b, at)
        at += 4
        for _ in range(self.n_ref):
            at += 8 + struct.unpack_from("<I", b, at)[0]
        self.first_record = at
        self._u_of = None

    def voff(self, u):
        """the virtual offset of inflated byte u: in the block that holds it; the end of a block is the start of the next one that
        holds bytes, and the end of all bytes the first block behind the last one that holds any"""
        import bisect
        if u >= len(self.data):
            k = max((i for i, n in enumerate(self.lens) if n), default=-1) + 1
            return self.block_at[k] << 16
        k = bisect.bisect_right(self.u_at, u) - 1
        while self.lens[k] == 0:
            k += 1
        return self.block_at[k] << 16 | (u - self.u_at[k])

    def u_of(self, v):
        """the inflated byte a virtual offset names"""
        if self._u_of is None:
            self._u_of = {}
            for at, u in zip(self.block_at, self.u_at):
                self._u_of.setdefault(at, u)
        return self._u_of[v >> 16] + (v & 0xffff)


def fields(b, at):
    """(size with block_size, refID, pos, end, flag) of the record at `at`, whose fixed fields, name and CIGAR lie inside b"""
    size, rid, pos, l_name, _mapq, _bin, n_cig, flag = struct.unpack_from("<IiiBBHHH", b, at)
    ref_len = 0
    for (w,) in struct.iter_unpack("<I", b[at + 36 + l_name:at + 36 + l_name + 4 * n_cig]):
        if bm.CIGAR_OPS[w & 15] in "MDN=X":
            ref_len += w >> 4
    return 4 + size, rid, pos, pos + max(1, ref_len), flag


def records(f):
    """[(inflated offset, size, refID, pos, end, flag)] of the chain of records; NotIndexable(MALFORMED, ...) where it breaks"""
    b, at, out = f.data, f.first_record, []
    while at < len(b):
        i = len(out) + 1
        if len(b) - at < 36:
            raise NotIndexable(MALFORMED, i)
        size, l_name, n_cig = struct.unpack_from("<I", b, at)[0], b[at + 12], struct.unpack_from("<H", b, at + 16)[0]
        if at + 4 + size > len(b) or size < 32 + l_name + 4 * n_cig:
            raise NotIndexable(MALFORMED, i)
        out.append((at,) + fields(b, at))
        at += 4 + size
    return out


def checked(f):
    """records(f), every one of them indexable: NotIndexable names the first that is not, and of its causes the one listed first"""
    recs = records(f)
    for i, (at, size, rid, pos, end, flag) in enumerate(recs):
        if rid < 0 or rid >= f.n_ref:
            raise NotIndexable(NOREF, i + 1)
        if i and (rid, pos) < recs[i - 1][2:4]:
            raise NotIndexable(UNSORTED, i + 1)
        if pos < 0 or end > MAX_END:
            raise NotIndexable(RANGE, i + 1)
    return recs


def model(file_bytes):
    """the .bai file's bytes for a whole BAM file"""
    f = File(bytes(file_bytes))
    recs = checked(f)
    refs = [{"raw": [], "lin": {}, "beg": None, "end": None, "mapped": 0, "unmapped": 0} for _ in range(f.n_ref)]
    before = None
    for at, size, rid, pos, end, flag in recs:
        r = refs[rid]
        key = (rid, bm.reg2bin(pos, end))
        vb, ve = f.voff(at), f.voff(at + size)
        if key == before:
            r["raw"][-1][2] = ve
        else:
            r["raw"].append([key[1], vb, ve])
        before = key
        for w in range(pos >> 14, ((end - 1) >> 14) + 1):
            r["lin"][w] = min(r["lin"].get(w, vb), vb)
        if r["beg"] is None:
            r["beg"] = vb
        r["end"] = ve
        r["unmapped" if flag & 4 else "mapped"] += 1
    o = [b"BAI\1", struct.pack("<I", f.n_ref)]
    for r in refs:
        if not r["raw"]:
            o.append(struct.pack("<II", 0, 0))
            continue
        bins = {}
        for b, vb, ve in r["raw"]:   # (file order within a bin)
            ch = bins.setdefault(b, [])
            if ch and vb >> 16 <= ch[-1][1] >> 16:
                ch[-1][1] = ve
            else:
                ch.append([vb, ve])
        o.append(struct.pack("<I", len(bins) + 1))
        for b in sorted(bins):
            o.append(struct.pack("<II", b, len(bins[b])) + b"".join(struct.pack("<QQ", *c) for c in bins[b]))
        o.append(struct.pack("<IIQQQQ", PSEUDO_BIN, 2, r["beg"], r["end"], r["mapped"], r["unmapped"]))
        n_intv = max(r["lin"]) + 1
        lin, nxt = [0] * n_intv, None
        for w in range(n_intv - 1, -1, -1):
            nxt = r["lin"].get(w, nxt)
            lin[w] = nxt
        o.append(struct.pack("<I", n_intv) + struct.pack("<%dQ" % n_intv, *lin))
    o.append(struct.pack("<Q", 0))
    return b"".join(o)


def parse_bai(payload):
    """[{"bins": {bin: [(beg, end)]}, "order": [bin], "pseudo": (beg, end, mapped, unmapped) or None, "lin": [offset]}], n_no_coor;
    every byte must be consumed"""
    p = bytes(payload)
    assert p[:4] == b"BAI\1", "no BAI magic"
    (n_ref,) = struct.unpack_from("<I", p, 4)
    at, refs = 8, []
    for _ in range(n_ref):
        (n_bin,) = struct.unpack_from("<i", p, at)
        at += 4
        r = {"bins": {}, "order": [], "pseudo": None, "lin": []}
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", p, at)
            at += 8
            ch = [struct.unpack_from("<QQ", p, at + 16 * k) for k in range(n_chunk)]
            at += 16 * n_chunk
            if b == PSEUDO_BIN:
                assert n_chunk == 2 and r["pseudo"] is None
                r["pseudo"] = ch[0] + ch[1]
            else:
                assert b < PSEUDO_BIN - 1 and b not in r["bins"] and n_chunk >= 1
                assert all(c[0] < c[1] for c in ch) and all(ch[k][1] <= ch[k + 1][0] for k in range(n_chunk - 1))
                r["bins"][b] = ch
                r["order"].append(b)
        (n_intv,) = struct.unpack_from("<i", p, at)
        at += 4
        r["lin"] = list(struct.unpack_from("<%dQ" % n_intv, p, at))
        at += 8 * n_intv
        refs.append(r)
    (n_no_coor,) = struct.unpack_from("<Q", p, at)
    assert at + 8 == len(p), "bytes behind the index"
    return refs, n_no_coor


def reg2bins(beg, end):
    """the bins a record that overlaps [beg, end) can lie in (SAM spec 5.3)"""
    end -= 1
    out = [0]
    for first, shift in ((1, 26), (9, 23), (73, 20), (585, 17), (4681, 14)):
        out.extend(range(first + (beg >> shift), first + (end >> shift) + 1))
    return out


def query(f, index, tid, beg, end):
    """the inflated offsets of the records of reference tid that overlap [beg, end), found through the parsed index: the chunks of
    the candidate bins that end behind the linear index's offset for beg's window, read from their first to their last byte"""
    r = index[tid]
    w = beg >> 14
    min_off = r["lin"][w] if w < len(r["lin"]) else (r["lin"][-1] if r["lin"] else 0)
    hits = set()
    for b in reg2bins(beg, end):
        for cb, ce in r["bins"].get(b, ()):
            if ce <= min_off:
                continue
            at, stop = f.u_of(cb), f.u_of(ce)
            while at < stop:
                size, rid, pos, rend, _ = fields(f.data, at)
                if rid == tid and pos < end and rend > beg:
                    hits.add(at)
                at += size
            assert at == stop, "a chunk that does not end with a record"
    return sorted(hits)


def brute(f, tid, beg, end):
    return [at for at, size, rid, pos, rend, _ in records(f) if rid == tid and pos < end and rend > beg]
