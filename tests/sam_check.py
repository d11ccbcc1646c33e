"""Per-record checks of SAM text against the reference sequence, shared by the fixture test (CPU) and the device test (GPU)."""
import re

import plain_align as pa

# records of the gap-rich SAM fixtures whose alignment the band (or ksw's gap-from-a-diagonal-move rule) keeps below the unbanded
# global optimum over their own span, by read name; at most 1 % of a fixture's records may be listed.  The reference's fixtures
# have none.
BAND_BINDING = {"x2_gaps_sam_q0": (), "x5_gaps_e15_sam_q0": (), "x6_gaps_se_sam_q0": ()}


def load_fasta(path):
    """{name: sequence bytes, case kept}"""
    seqs, name, cur = {}, None, []
    with open(path, "rb") as f:
        for line in f:
            if line.startswith(b">"):
                if name is not None:
                    seqs[name] = b"".join(cur)
                name, cur = line[1:].split()[0], []
            else:
                cur.append(line.strip())
    if name is not None:
        seqs[name] = b"".join(cur)
    return seqs


def records(text):
    """mapped records of SAM text: dicts with name, flag, rname, pos (0-based), ops, seq, nm, md"""
    out = []
    for line in text.split(b"\n"):
        if not line or line.startswith(b"@"):
            continue
        f = line.split(b"\t")
        if f[5] == b"*":
            continue
        tags = {t[:2]: t[5:] for t in f[11:]}
        out.append({"name": f[0].decode(), "flag": int(f[1]), "rname": f[2], "pos": int(f[3]) - 1, "ops": pa.parse_cigar(f[5]),
                    "seq": f[9], "nm": int(tags[b"NM"]), "md": tags[b"MD"].decode()})
    return out


def check_record(rec, ref):
    """replay accepts the CIGAR against exactly the span it reports, and NM / MD recomputed from scratch equal the text.
    Returns (affine score of the CIGAR, reference span)."""
    span_len = sum(n for op, n in rec["ops"] if op in "MD")
    chrom = ref[rec["rname"]]
    assert 0 <= rec["pos"] and rec["pos"] + span_len <= len(chrom), "%s: span outside %s" % (rec["name"], rec["rname"].decode())
    span = chrom[rec["pos"]:rec["pos"] + span_len]
    try:
        score, nm, md = pa.replay(rec["ops"], span, rec["seq"])
    except AssertionError as ex:
        raise AssertionError("%s (flag %d): %s" % (rec["name"], rec["flag"], ex))
    assert nm == rec["nm"], "%s (flag %d): NM %d in the text, %d recomputed" % (rec["name"], rec["flag"], rec["nm"], nm)
    assert md == rec["md"], "%s (flag %d): MD %s in the text, %s recomputed" % (rec["name"], rec["flag"], rec["md"], md)
    return score, span


def gap_profile(rec):
    """(has a gap, has a gap run of 2 or more bases, has a gap within 3 read positions of either end of the read)"""
    ops = rec["ops"]
    gaps = [(op, n) for op, n in ops if op in "ID"]
    near = False
    rp, total = 0, sum(n for op, n in ops if op in "MIS")
    for op, n in ops:
        if op in "ID" and (rp <= 3 or total - (rp + (n if op == "I" else 0)) <= 3):
            near = True
        if op in "MIS":
            rp += n
    return bool(gaps), any(n >= 2 for _, n in gaps), near


def check_cut_record(rec):
    """a split-aligned record prints SEQ cut to the CIGAR's query length, not the aligned bases themselves, so it cannot be
    replayed against the reference from the SAM line alone.  What the line must still satisfy: M + I (+ S) = len(SEQ); the MD
    string covers exactly the M and D bases (matches + mismatches = M, bases after ^ = D, one ^ run per D operation in order);
    NM = mismatches in MD + inserted + deleted bases."""
    ops = rec["ops"]
    m, i, d = (sum(n for op, n in ops if op == k) for k in "MID")
    s = sum(n for op, n in ops if op == "S")
    assert all(n > 0 for _, n in ops) and all(a[0] != b[0] for a, b in zip(ops, ops[1:])), rec["name"]
    assert m + i + s == len(rec["seq"]), "%s: CIGAR query length %d, SEQ %d" % (rec["name"], m + i + s, len(rec["seq"]))
    tokens = re.findall(r"\d+|\^[A-Za-z]+|[A-Za-z]", rec["md"])
    assert "".join(tokens) == rec["md"] and tokens and tokens[0].isdigit() and tokens[-1].isdigit(), "%s: MD %s" % (rec["name"], rec["md"])
    matches = sum(int(t) for t in tokens if t.isdigit())
    mism = sum(1 for t in tokens if t.isalpha())
    dels = [len(t) - 1 for t in tokens if t[0] == "^"]
    assert matches + mism == m, "%s: MD covers %d aligned bases, the CIGAR %d" % (rec["name"], matches + mism, m)
    assert dels == [n for op, n in ops if op == "D"], "%s: MD deletions %s against CIGAR %s" % (rec["name"], dels, ops)
    assert rec["nm"] == mism + i + d, "%s: NM %d, MD and CIGAR give %d" % (rec["name"], rec["nm"], mism + i + d)
