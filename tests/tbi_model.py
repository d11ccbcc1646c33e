"""The tabix index of a sorted BED-like text as chromap_amd writes it (cmgpu_bgzf_index_tabix), built line by line from the rules of the
SAM/tabix specification; a reader of the format written from the same specification; and a brute-force region query.  Pure Python, no
device.  Test infrastructure only."""
import struct
import zlib

SLICE = 0xff00
MAX_END = 1 << 29
PSEUDO_BIN = 37450
HEADER = struct.pack("<4s7i", b"TBI\1", 0, 0x10000, 1, 2, 3, 35, 0)  # (n_ref is patched in)


class NotIndexable(ValueError):
    """the text breaks one of the indexer's rules; .line is the 1-based number of the first offending line, .cause a short word"""

    def __init__(self, cause, line):
        ValueError.__init__(self, "%s at line %d" % (cause, line))
        self.cause, self.line = cause, line


def reg2bin(beg, end):
    end -= 1
    if beg >> 14 == end >> 14:
        return 4681 + (beg >> 14)
    if beg >> 17 == end >> 17:
        return 585 + (beg >> 17)
    if beg >> 20 == end >> 20:
        return 73 + (beg >> 20)
    if beg >> 23 == end >> 23:
        return 9 + (beg >> 23)
    if beg >> 26 == end >> 26:
        return 1 + (beg >> 26)
    return 0


def reg2bins(beg, end):
    end -= 1
    out = [0]
    for first, shift in ((1, 26), (9, 23), (73, 20), (585, 17), (4681, 14)):
        out.extend(range(first + (beg >> shift), first + (end >> shift) + 1))
    return out


def block_sizes(blocks):
    """[(offset, size)] (bgzf_texts.blocks) or plain sizes -> sizes"""
    return [b[1] if isinstance(b, tuple) else b for b in blocks]


def _digits(col):
    return len(col) > 0 and all(48 <= c <= 57 for c in col)


def parse_lines(text):
    """[(name, beg, end, start offset, end offset)] with end already made beg + 1 where it was not larger; raises NotIndexable"""
    if text and not text.endswith(b"\n"):
        raise NotIndexable("no final newline", text.count(b"\n") + 1)
    out = []
    at = 0
    no = 0
    while at < len(text):
        nl = text.index(b"\n", at)
        no += 1
        cols = text[at:nl].split(b"\t", 3)
        if len(cols) < 3 or not cols[0] or not _digits(cols[1]) or not _digits(cols[2]):
            raise NotIndexable("malformed", no)
        beg, end = int(cols[1]), int(cols[2])
        if end <= beg:
            end = beg + 1
        if end > MAX_END:
            raise NotIndexable("beyond 2^29", no)
        out.append((cols[0], beg, end, at, nl + 1))
        at = nl + 1
    return out


def model(text, blocks, base):
    """the index payload (the .tbi before compression) of `text` whose slices of 0xff00 bytes became BGZF blocks of the given sizes,
    the first of them at file offset `base`"""
    sizes = block_sizes(blocks)
    assert len(sizes) == (len(text) + SLICE - 1) // SLICE
    coff = [0]
    for s in sizes:
        coff.append(coff[-1] + s)

    def voff(u):
        if u == len(text):
            return (base + coff[len(sizes)]) << 16
        return ((base + coff[u // SLICE]) << 16) | (u % SLICE)

    lines = parse_lines(text)
    refs = []   # [name, {bin: [[beg, end], ...]}, ioff dict, n_intv, first voff, last voff, lines]
    seen = set()
    prev = None
    for no, (name, beg, end, u0, u1) in enumerate(lines, 1):
        if prev is None or name != prev[0]:
            if name in seen:
                raise NotIndexable("name recurs", no)
            seen.add(name)
            refs.append([name, {}, {}, 0, voff(u0), 0, 0])
            last_bin = None
        elif beg < prev[1]:
            raise NotIndexable("not sorted", no)
        r = refs[-1]
        b = reg2bin(beg, end)
        if b != last_bin:
            r[1].setdefault(b, []).append([voff(u0), voff(u1)])   # a raw chunk begins
            cur = r[1][b][-1]
            last_bin = b
        else:
            cur[1] = voff(u1)
        for w in range(beg >> 14, ((end - 1) >> 14) + 1):
            if w not in r[2] or voff(u0) < r[2][w]:
                r[2][w] = voff(u0)
        r[3] = max(r[3], ((end - 1) >> 14) + 1)
        r[5] = voff(u1)
        r[6] += 1
        prev = (name, beg)
    out = bytearray(HEADER)
    struct.pack_into("<i", out, 4, len(refs))
    names = b"".join(r[0] + b"\0" for r in refs)
    out += struct.pack("<i", len(names)) + names
    stats = {"raw": 0, "merged": 0}
    for name, bins, lin, n_intv, v0, v1, n_lines in refs:
        out += struct.pack("<i", len(bins) + 1)
        for b in sorted(bins):
            chunks = sorted(bins[b])
            stats["raw"] += len(chunks)
            merged = [list(chunks[0])]
            for c in chunks[1:]:
                if c[0] >> 16 <= merged[-1][1] >> 16:
                    merged[-1][1] = c[1]
                else:
                    merged.append(list(c))
            stats["merged"] += len(merged)
            out += struct.pack("<Ii", b, len(merged))
            for c in merged:
                out += struct.pack("<QQ", c[0], c[1])
        out += struct.pack("<Ii4Q", PSEUDO_BIN, 2, v0, v1, n_lines, 0)
        ioff = [lin.get(w) for w in range(n_intv)]
        for w in range(n_intv - 2, -1, -1):
            if ioff[w] is None:
                ioff[w] = ioff[w + 1]
        out += struct.pack("<i", n_intv) + struct.pack("<%dQ" % n_intv, *ioff)
    out += struct.pack("<Q", 0)
    model.last_stats = stats
    return bytes(out)


def parse_tbi(payload):
    """{'names': [...], 'refs': [{'bins': {bin: [(beg, end)]}, 'ioff': [...]}], 'n_no_coor': int}; the whole payload must be used up"""
    magic, n_ref, fmt, cs, cb, ce, meta, skip, l_nm = struct.unpack_from("<4s8i", payload, 0)
    assert magic == b"TBI\1" and (fmt, cs, cb, ce, meta, skip) == (0x10000, 1, 2, 3, 35, 0)
    at = 36
    blob = payload[at:at + l_nm]
    at += l_nm
    names = blob.split(b"\0")[:-1] if l_nm else []
    assert len(names) == n_ref and (l_nm == 0 or blob.endswith(b"\0"))
    refs = []
    for _ in range(n_ref):
        (n_bin,) = struct.unpack_from("<i", payload, at)
        at += 4
        bins = {}
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", payload, at)
            at += 8
            assert b not in bins
            bins[b] = [struct.unpack_from("<QQ", payload, at + 16 * i) for i in range(n_chunk)]
            at += 16 * n_chunk
        (n_intv,) = struct.unpack_from("<i", payload, at)
        at += 4
        ioff = list(struct.unpack_from("<%dQ" % n_intv, payload, at))
        at += 8 * n_intv
        refs.append({"bins": bins, "ioff": ioff})
    (n_no_coor,) = struct.unpack_from("<Q", payload, at)
    assert at + 8 == len(payload)
    return {"names": names, "refs": refs, "n_no_coor": n_no_coor}


class _Reader:
    """reads a BGZF file by virtual offset, one block at a time"""

    def __init__(self, raw):
        self.raw = raw
        self.cache = {}

    def block(self, coff):
        if coff not in self.cache:
            raw = self.raw
            assert raw[coff:coff + 4] == b"\x1f\x8b\x08\x04", "a virtual offset that points at no block"
            size = struct.unpack_from("<H", raw, coff + 16)[0] + 1
            data = zlib.decompress(raw[coff + 18:coff + size - 8], -15)
            self.cache[coff] = (data, coff + size)
        return self.cache[coff]

    def lines(self, vbeg, vend):
        """the lines that start in [vbeg, vend)"""
        coff, uoff = vbeg >> 16, vbeg & 0xffff
        line = bytearray()
        while coff < len(self.raw):
            data, nxt = self.block(coff)
            if uoff >= len(data):
                coff, uoff = nxt, 0
                continue
            if not line and ((coff << 16) | uoff) >= vend:
                return
            nl = data.find(b"\n", uoff)
            if nl < 0:
                line += data[uoff:]
                coff, uoff = nxt, 0
                continue
            line += data[uoff:nl + 1]
            uoff = nl + 1
            yield bytes(line)
            line = bytearray()
        assert not line


def query(raw_bgzf, index, name, beg, end):
    """the lines of the BGZF file `raw_bgzf` that overlap name:[beg, end), in file order, found through `index` (a parse_tbi result)"""
    if name not in index["names"] or beg >= end:
        return []
    ref = index["refs"][index["names"].index(name)]
    ioff = ref["ioff"]
    if not ioff:
        return []
    w = beg >> 14
    min_off = ioff[w] if w < len(ioff) else ioff[-1]
    chunks = []
    for b in reg2bins(beg, min(end, MAX_END)):
        if b == PSEUDO_BIN:
            continue
        for c in ref["bins"].get(b, ()):
            if c[1] > min_off:
                chunks.append(c)
    chunks.sort()
    merged = []
    for c in chunks:
        if merged and c[0] <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], c[1])
        else:
            merged.append(list(c))
    rd = _Reader(raw_bgzf)
    out = []
    for vb, ve in merged:
        for line in rd.lines(vb, ve):
            cols = line.rstrip(b"\n").split(b"\t")
            if cols[0] != name:
                continue
            b0, e0 = int(cols[1]), int(cols[2])
            if e0 <= b0:
                e0 = b0 + 1
            if b0 < end and e0 > beg:
                out.append(line)
    return out


def brute(text, name, beg, end):
    out = []
    for line in text.splitlines(True):
        cols = line.rstrip(b"\n").split(b"\t")
        if cols[0] != name:
            continue
        b0, e0 = int(cols[1]), int(cols[2])
        if e0 <= b0:
            e0 = b0 + 1
        if b0 < end and e0 > beg:
            out.append(line)
    return out
