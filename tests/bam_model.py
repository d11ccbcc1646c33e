"""BAM (SAM specification, section 4.2) in plain Python, for the tests of the device's BAM writer (chromap_amd/csrc/cm_bam.h):
encode() makes the uncompressed header and alignment records of a SAM text, decode() prints uncompressed BAM bytes as SAM text.
The two share the constants below and nothing else: neither calls the other.  Test infrastructure only."""
import struct

SEQ_ALPHABET = "=ACMGRSVTWYHKDBN"
CIGAR_OPS = "MIDNSHP=X"


def reg2bin(beg, end):
    """the specification's function for the 0-based half-open interval [beg, end)"""
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def normalise(sam_text):
    """the SAM text as a BAM file can hold it: SEQ upper-cased, and N where the 4-bit alphabet has no letter"""
    out = []
    for ln in sam_text.split(b"\n"):
        if ln and not ln.startswith(b"@"):
            c = ln.split(b"\t")
            c[9] = bytes(x if chr(x) in SEQ_ALPHABET else ord("N") for x in c[9].upper())
            ln = b"\t".join(c)
        out.append(ln)
    return b"\n".join(out)


def _split(sam_text):
    lines = [ln for ln in sam_text.split(b"\n") if ln]
    return [ln for ln in lines if ln.startswith(b"@")], [ln for ln in lines if not ln.startswith(b"@")]


def _tag(field):
    tag, typ, val = field.split(b":", 2)
    assert len(tag) == 2
    if typ == b"Z":
        return tag + b"Z" + val + b"\0"
    if typ == b"A":
        return tag + b"A" + val
    if typ == b"f":
        return tag + b"f" + struct.pack("<f", float(val))
    assert typ == b"i", field
    v = int(val)
    if v >= 0:  # the smallest type that holds the value, unsigned first: samtools' choice
        return tag + (b"C" + struct.pack("<B", v) if v < 256 else b"S" + struct.pack("<H", v) if v < 65536 else b"I" + struct.pack("<I", v))
    return tag + (b"c" + struct.pack("<b", v) if v >= -128 else b"s" + struct.pack("<h", v) if v >= -32768 else b"i" + struct.pack("<i", v))


def encode_record(line, ref_ids):
    c = line.split(b"\t")
    qname, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, qual = c[:11]
    name = b"" if qname == b"*" else qname
    assert len(name) <= 254, "l_read_name is one byte and counts the NUL"
    rid = -1 if rname == b"*" else ref_ids[rname]
    nrid = -1 if rnext == b"*" else rid if rnext == b"=" else ref_ids[rnext]
    words, num, ref_len = [], 0, 0
    if cigar != b"*":
        for ch in cigar.decode():
            if ch.isdigit():
                num = num * 10 + int(ch)
            else:
                op = CIGAR_OPS.index(ch)
                words.append(num << 4 | op)
                if ch in "MDN=X":
                    ref_len += num
                num = 0
    beg = int(pos) - 1
    if seq == b"*":
        seq = b""
    nib = [SEQ_ALPHABET.index(ch) if ch in SEQ_ALPHABET else 15 for ch in seq.decode("latin-1").upper()]
    if len(nib) & 1:
        nib.append(0)
    packed = bytes(nib[i] << 4 | nib[i + 1] for i in range(0, len(nib), 2))
    q = b"\xff" * len(seq) if qual == b"*" else bytes((x - 33) & 0xff for x in qual)
    assert len(q) == len(seq)
    body = struct.pack("<iiBBHHHIiii", rid, beg, len(name) + 1, int(mapq), reg2bin(beg, beg + (ref_len or 1)), len(words), int(flag), len(seq),
                       nrid, int(pnext) - 1, int(tlen))
    body += name + b"\0" + struct.pack("<%dI" % len(words), *words) + packed + q + b"".join(_tag(f) for f in c[11:])
    return struct.pack("<I", len(body)) + body


def encode(sam_text):
    """(header bytes, record bytes) of a SAM text whose header lines include one @SQ per sequence"""
    head, recs = _split(sam_text)
    refs = []
    for ln in head:
        if ln.startswith(b"@SQ"):
            f = dict(x.split(b":", 1) for x in ln.split(b"\t")[1:])
            refs.append((f[b"SN"], int(f[b"LN"])))
    text = b"".join(ln + b"\n" for ln in head)
    header = b"BAM\1" + struct.pack("<I", len(text)) + text + struct.pack("<I", len(refs))
    for nm, ln in refs:
        header += struct.pack("<I", len(nm) + 1) + nm + b"\0" + struct.pack("<I", ln)
    ref_ids = {nm: i for i, (nm, _) in enumerate(refs)}
    return header, b"".join(encode_record(ln, ref_ids) for ln in recs)


def decode(bam_bytes):
    """the SAM text (header text, then one line per record) of uncompressed BAM bytes"""
    b = bytes(bam_bytes)
    assert b[:4] == b"BAM\1", "no BAM magic"
    (l_text,) = struct.unpack_from("<I", b, 4)
    at = 8 + l_text
    out = [b[8:at].rstrip(b"\0")]
    (n_ref,) = struct.unpack_from("<I", b, at)
    at += 4
    names = []
    for _ in range(n_ref):
        (l_name,) = struct.unpack_from("<I", b, at)
        assert b[at + 4 + l_name - 1] == 0
        names.append(b[at + 4:at + 4 + l_name - 1])
        at += 4 + l_name + 4
    while at < len(b):
        (size,) = struct.unpack_from("<I", b, at)
        end = at + 4 + size
        assert end <= len(b), "record runs past the end"
        rid, pos, l_name, mapq, bin_, n_cig, flag, l_seq, nrid, npos, tlen = struct.unpack_from("<iiBBHHHIiii", b, at + 4)
        p = at + 36
        assert b[p + l_name - 1] == 0
        qname = b[p:p + l_name - 1] or b"*"
        p += l_name
        cig, ref_len = "", 0
        for w in struct.unpack_from("<%dI" % n_cig, b, p):
            cig += "%d%s" % (w >> 4, CIGAR_OPS[w & 15])
            if CIGAR_OPS[w & 15] in "MDN=X":
                ref_len += w >> 4
        p += 4 * n_cig
        assert bin_ == reg2bin(pos, pos + (ref_len or 1)), "bin"
        seq = "".join(SEQ_ALPHABET[b[p + i // 2] >> 4 if i % 2 == 0 else b[p + i // 2] & 15] for i in range(l_seq))
        assert l_seq % 2 == 0 or b[p + l_seq // 2] & 15 == 0, "the padding nibble"
        p += (l_seq + 1) // 2
        raw = b[p:p + l_seq]
        qual = b"*" if l_seq and raw == b"\xff" * l_seq else bytes(x + 33 for x in raw)
        p += l_seq
        tags = []
        while p < end:
            tag, typ = b[p:p + 2], chr(b[p + 2])
            p += 3
            if typ == "Z":
                z = b.index(b"\0", p)
                assert z < end
                tags.append(tag + b":Z:" + b[p:z])
                p = z + 1
            elif typ == "A":
                tags.append(tag + b":A:" + b[p:p + 1])
                p += 1
            else:
                fmt = {"C": "<B", "c": "<b", "S": "<H", "s": "<h", "I": "<I", "i": "<i"}[typ]
                tags.append(tag + b":i:%d" % struct.unpack_from(fmt, b, p))
                p += struct.calcsize(fmt)
        assert p == end, "tags do not end with the record"
        rname = names[rid] if rid >= 0 else b"*"
        rnext = b"*" if nrid < 0 else b"=" if nrid == rid else names[nrid]
        cols = [qname, b"%d" % flag, rname, b"%d" % (pos + 1), b"%d" % mapq, cig.encode() or b"*", rnext, b"%d" % (npos + 1), b"%d" % tlen,
                seq.encode() or b"*", qual or b"*"] + tags
        out.append(b"\t".join(cols) + b"\n")
        at = end
    return b"".join(out)
