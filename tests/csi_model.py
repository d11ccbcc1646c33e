"""The CSI index (.csi; SAM specification 5.3, CSIv1) in plain Python, written from the specification: min_shift 14, `depth` levels,
every bin with its chunks of virtual offsets and its loffset, the pseudo-bin ((1 << (3 * depth + 3)) - 1) / 7 + 1, no linear index;
and from the rules the device's builder states for what the specification leaves open (chromap_amd/csrc/cm_tabix.h, cm_bai.h): the
chunk rules of the .tbi / .bai (tests/tbi_model.py, tests/bai_model.py), bins not folded, a bin's loffset the back-filled 16 kb window
value at the bin's first position (htslib's rule), the pseudo-bin's 0, positions of 32 bits (depth 6 takes ends up to 0xffffffff).
Two flavours: BAM (no aux; the input is a whole BAM file) and tabix (aux: the tabix header behind its magic and n_ref; the input is a
BED text and its block table).  Also a reader of the format and region queries through it that follow the specification's reader:
reg2bins for any depth, and min_off from the loffset of the leaf bin of the region's start, or of the nearest bin before it among
its previous siblings and its ancestors.  Test infrastructure only."""
import bisect
import struct

import bai_model as bai
import tbi_model as tm

MIN_SHIFT = 14
MALFORMED, NOREF, UNSORTED, RANGE = bai.MALFORMED, bai.NOREF, bai.UNSORTED, bai.RANGE
TABIX_AUX_HEAD = struct.pack("<6i", 0x10000, 1, 2, 3, 35, 0)


def max_end(depth):
    return min(1 << (MIN_SHIFT + 3 * depth), 0xffffffff)


def pseudo_bin(depth):
    return ((1 << (3 * depth + 3)) - 1) // 7 + 1


def level_first(level):
    """the first bin of a level (level 0: bin 0)"""
    return ((1 << (3 * level)) - 1) // 7


def reg2bin(beg, end, depth):
    """the specification's reg2bin(beg, end, min_shift = 14, depth)"""
    end -= 1
    s, t = MIN_SHIFT, level_first(depth)
    for l in range(depth, 0, -1):
        if beg >> s == end >> s:
            return t + (beg >> s)
        s += 3
        t -= 1 << (3 * (l - 1))
    return 0


def reg2bins(beg, end, depth):
    """the specification's reg2bins: every bin a record that overlaps [beg, end) can lie in"""
    end -= 1
    out = []
    s = MIN_SHIFT + 3 * depth
    for l in range(depth + 1):
        t = level_first(l)
        out.extend(range(t + (beg >> s), t + (end >> s) + 1))
        s -= 3
    return out


def bin_level(b):
    l = 0
    while b >= level_first(l + 1):
        l += 1
    return l


def bin_begin(b, depth):
    """the first position of bin b"""
    l = bin_level(b)
    return (b - level_first(l)) << (MIN_SHIFT + 3 * (depth - l))


def bin_parent(b):
    return (b - 1) >> 3


# ---- the builder: items (reference, beg, end, vbeg, vend, unmapped) in file order
def _build(n_ref, items, depth):
    refs = [{"raw": [], "lin": {}, "beg": None, "end": None, "mapped": 0, "unmapped": 0} for _ in range(n_ref)]
    before = None
    for rid, beg, end, vb, ve, unm in items:
        r = refs[rid]
        key = (rid, reg2bin(beg, end, depth))
        if key == before:
            r["raw"][-1][2] = ve
        else:
            r["raw"].append([key[1], vb, ve])
        before = key
        for w in range(beg >> MIN_SHIFT, ((end - 1) >> MIN_SHIFT) + 1):
            r["lin"][w] = min(r["lin"].get(w, vb), vb)
        if r["beg"] is None:
            r["beg"] = vb
        r["end"] = ve
        r["unmapped" if unm else "mapped"] += 1
    return refs


def _serialize(depth, aux, refs):
    o = [b"CSI\1", struct.pack("<iii", MIN_SHIFT, depth, len(aux)), aux, struct.pack("<i", len(refs))]
    for r in refs:
        if not r["raw"]:
            o.append(struct.pack("<i", 0))
            continue
        bins = {}
        for b, vb, ve in r["raw"]:   # (file order within a bin)
            ch = bins.setdefault(b, [])
            if ch and vb >> 16 <= ch[-1][1] >> 16:
                ch[-1][1] = ve
            else:
                ch.append([vb, ve])
        # the windows, filled from the right
        lin, filled = r["lin"], sorted(r["lin"])

        def window(w):
            k = bisect.bisect_left(filled, w)
            assert k < len(filled), "a bin whose first window lies behind its reference's last record"
            return lin[filled[k]]
        o.append(struct.pack("<i", len(bins) + 1))
        for b in sorted(bins):
            o.append(struct.pack("<IQi", b, window(bin_begin(b, depth) >> MIN_SHIFT), len(bins[b])) + b"".join(struct.pack("<QQ", *c) for c in bins[b]))
        o.append(struct.pack("<IQiQQQQ", pseudo_bin(depth), 0, 2, r["beg"], r["end"], r["mapped"], r["unmapped"]))
    o.append(struct.pack("<Q", 0))
    return b"".join(o)


# ---- the BAM flavour
def bam_checked(f, depth):
    """bai_model.checked with the depth's limit"""
    recs = bai.records(f)
    for i, (at, size, rid, pos, end, flag) in enumerate(recs):
        if rid < 0 or rid >= f.n_ref:
            raise bai.NotIndexable(NOREF, i + 1)
        if i and (rid, pos) < recs[i - 1][2:4]:
            raise bai.NotIndexable(UNSORTED, i + 1)
        if pos < 0 or end > max_end(depth):
            raise bai.NotIndexable(RANGE, i + 1)
    return recs


def bam_model(file_bytes, depth):
    """the CSI payload (the .csi before compression) for a whole BAM file"""
    f = bai.File(bytes(file_bytes))
    items = [(rid, pos, end, f.voff(at), f.voff(at + size), flag & 4) for at, size, rid, pos, end, flag in bam_checked(f, depth)]
    return _serialize(depth, b"", _build(f.n_ref, items, depth))


# ---- the tabix flavour
def bed_lines(text, depth):
    """tbi_model.parse_lines with the depth's limit"""
    if text and not text.endswith(b"\n"):
        raise tm.NotIndexable("no final newline", text.count(b"\n") + 1)
    out, at, no = [], 0, 0
    while at < len(text):
        nl = text.index(b"\n", at)
        no += 1
        cols = text[at:nl].split(b"\t", 3)
        if len(cols) < 3 or not cols[0] or not tm._digits(cols[1]) or not tm._digits(cols[2]):
            raise tm.NotIndexable("malformed", no)
        beg, end = int(cols[1]), int(cols[2])
        if end <= beg:
            end = beg + 1
        if end > max_end(depth):
            raise tm.NotIndexable("beyond the limit", no)
        out.append((cols[0], beg, end, at, nl + 1))
        at = nl + 1
    return out


def bed_model(text, blocks, base, depth):
    """the CSI payload of `text` whose slices of 0xff00 bytes became BGZF blocks of the given sizes, the first at file offset `base`"""
    sizes = tm.block_sizes(blocks)
    assert len(sizes) == (len(text) + tm.SLICE - 1) // tm.SLICE
    coff = [0]
    for s in sizes:
        coff.append(coff[-1] + s)

    def voff(u):
        if u == len(text):
            return (base + coff[len(sizes)]) << 16
        return ((base + coff[u // tm.SLICE]) << 16) | (u % tm.SLICE)

    names, items, seen, prev = [], [], set(), None
    for no, (name, beg, end, u0, u1) in enumerate(bed_lines(text, depth), 1):
        if prev is None or name != prev[0]:
            if name in seen:
                raise tm.NotIndexable("name recurs", no)
            seen.add(name)
            names.append(name)
        elif beg < prev[1]:
            raise tm.NotIndexable("not sorted", no)
        items.append((len(names) - 1, beg, end, voff(u0), voff(u1), 0))
        prev = (name, beg)
    blob = b"".join(n + b"\0" for n in names)
    return _serialize(depth, TABIX_AUX_HEAD + struct.pack("<i", len(blob)) + blob, _build(len(names), items, depth))


# ---- the reader
def parse_csi(payload):
    """{"depth", "aux", "names" (tabix flavour, else None), "refs": [{"bins": {bin: [(beg, end)]}, "loff": {bin: loffset}, "order": [bin],
    "pseudo": (beg, end, mapped, unmapped) or None}], "n_no_coor"}; every byte must be consumed"""
    p = bytes(payload)
    assert p[:4] == b"CSI\1", "no CSI magic"
    min_shift, depth, l_aux = struct.unpack_from("<iii", p, 4)
    assert min_shift == MIN_SHIFT and 1 <= depth <= 6 and l_aux >= 0
    aux = p[16:16 + l_aux]
    at = 16 + l_aux
    names = None
    if l_aux:
        assert aux[:24] == TABIX_AUX_HEAD
        (l_nm,) = struct.unpack_from("<i", aux, 24)
        assert l_aux == 28 + l_nm and (l_nm == 0 or aux.endswith(b"\0"))
        names = aux[28:].split(b"\0")[:-1] if l_nm else []
    (n_ref,) = struct.unpack_from("<i", p, at)
    at += 4
    assert names is None or len(names) == n_ref
    refs = []
    for _ in range(n_ref):
        (n_bin,) = struct.unpack_from("<i", p, at)
        at += 4
        r = {"bins": {}, "loff": {}, "order": [], "pseudo": None}
        for _ in range(n_bin):
            b, loff, n_chunk = struct.unpack_from("<IQi", p, at)
            at += 16
            ch = [struct.unpack_from("<QQ", p, at + 16 * k) for k in range(n_chunk)]
            at += 16 * n_chunk
            if b == pseudo_bin(depth):
                assert n_chunk == 2 and r["pseudo"] is None and loff == 0
                r["pseudo"] = ch[0] + ch[1]
            else:
                assert b < pseudo_bin(depth) - 1 and b not in r["bins"] and n_chunk >= 1
                assert all(c[0] < c[1] for c in ch) and all(ch[k][1] <= ch[k + 1][0] for k in range(n_chunk - 1))
                assert loff != 0xffffffffffffffff and loff <= ch[0][0]
                r["bins"][b] = ch
                r["loff"][b] = loff
                r["order"].append(b)
        assert r["order"] == sorted(r["order"]) and (r["pseudo"] is not None) == (n_bin > 0)
        refs.append(r)
    (n_no_coor,) = struct.unpack_from("<Q", p, at)
    assert at + 8 == len(p), "bytes behind the index"
    return {"depth": depth, "aux": aux, "names": names, "refs": refs, "n_no_coor": n_no_coor}


def min_off(ref, beg, depth):
    """the specification's reader: the loffset of the leaf bin of `beg` or, where that bin is not there, of the nearest bin before
    it -- its previous siblings, then its parent, and so on up; 0 where none is there"""
    b = level_first(depth) + (min(beg, max_end(depth) - 1) >> MIN_SHIFT)
    while True:
        if b in ref["loff"]:
            return ref["loff"][b]
        if b == 0:
            return 0
        first = (bin_parent(b) << 3) + 1
        b = b - 1 if b > first else bin_parent(b)


def chunks_for(ref, beg, end, depth):
    """the chunks a reader has to read for [beg, end): those of the candidate bins that end behind min_off"""
    lo = min_off(ref, beg, depth)
    return [c for b in reg2bins(beg, min(end, max_end(depth)), depth) for c in ref["bins"].get(b, ()) if c[1] > lo], lo


def query_bam(f, index, tid, beg, end):
    """the inflated offsets of the records of reference tid that overlap [beg, end), found through the parsed index: read from each
    chunk's first to its last byte, the records at or behind min_off"""
    hits = set()
    if beg >= max_end(index["depth"]):
        return []
    chunks, lo = chunks_for(index["refs"][tid], beg, end, index["depth"])
    for cb, ce in chunks:
        at, stop = f.u_of(cb), f.u_of(ce)
        while at < stop:
            size, rid, pos, rend, _ = bai.fields(f.data, at)
            if rid == tid and pos < end and rend > beg and f.voff(at) >= lo:
                hits.add(at)
            at += size
        assert at == stop, "a chunk that does not end with a record"
    return sorted(hits)


def query_bed(raw_bgzf, index, name, beg, end):
    """the lines of the BGZF file that overlap name:[beg, end), in file order, found through the parsed index"""
    if name not in index["names"] or beg >= end or beg >= max_end(index["depth"]):
        return []
    chunks, lo = chunks_for(index["refs"][index["names"].index(name)], beg, end, index["depth"])
    merged = []
    for c in sorted(chunks):
        c = (max(c[0], lo), c[1])   # (nothing before min_off is read)
        if merged and c[0] <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], c[1])
        else:
            merged.append(list(c))
    rd = tm._Reader(raw_bgzf)
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


def check_bed_queries(raw, payload, text, queries):
    """every query through the index returns what a scan of the text returns"""
    idx = parse_csi(payload)
    table = {}
    for ln in text.splitlines(True):
        cols = ln.split(b"\t", 3)
        b, e = int(cols[1]), int(cols[2])
        table.setdefault(cols[0], []).append((b, e if e > b else b + 1, ln))
    found = 0
    for name, beg, end in queries:
        want = [ln for b, e, ln in table.get(name, ()) if b < end and e > beg]
        assert query_bed(raw, idx, name, beg, end) == want, (name, beg, end)
        found += len(want)
    return found


def check_bam_queries(raw, payload, regions):
    f = bai.File(raw)
    idx = parse_csi(payload)
    assert idx["n_no_coor"] == 0 and len(idx["refs"]) == f.n_ref and idx["names"] is None
    found = 0
    for tid, beg, end in regions:
        want = bai.brute(f, tid, beg, end)
        assert query_bam(f, idx, tid, beg, end) == want, (tid, beg, end)
        found += len(want)
    return found
