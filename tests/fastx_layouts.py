"""What the record layouts of FASTA / FASTQ text mean, for the tests of layout CMGPU_FASTX_FREE: a byte-level model of the reference's
reader (kseq_read plus the skip of empty records, written from the description in include/chromap_amd.h), hand-made texts, and two seeded
generators -- one restricted to what the device ingest must accept, one wild."""
import random

SPACE = b" \t\n\v\f\r"


class Kseq:
    """kseq_read over a byte string.  records(): ([(name, seq, qual or None), ...], truncated) -- records with an empty sequence are
    dropped as the reference's batch loader drops them; truncated: the reader gave up with "truncated quality" (-2)."""

    def __init__(self, text):
        self.t, self.p, self.pending = bytes(text), 0, False  # pending: a header marker has been read already

    def _getc(self):
        if self.p >= len(self.t):
            return -1
        self.p += 1
        return self.t[self.p - 1]

    def _line(self, buf):
        """appends the rest of the line to buf and drops ONE trailing CR if buf is then longer than one byte; False: nothing left to read"""
        if self.p >= len(self.t):
            return False
        e = self.t.find(b"\n", self.p)
        if e < 0:
            buf += self.t[self.p:]
            self.p = len(self.t)
        else:
            buf += self.t[self.p:e]
            self.p = e + 1
        if len(buf) > 1 and buf[-1] == 13:
            del buf[-1]
        return True

    def read(self):
        """one record: (name, seq, qual or None), None at the end of the text, -2 for a truncated quality"""
        if not self.pending:
            while True:
                c = self._getc()
                if c < 0:
                    return None
                if c in b"@>":
                    break
            self.pending = True
        if self.p >= len(self.t):
            return None
        s = self.p
        while self.p < len(self.t) and self.t[self.p] not in SPACE:
            self.p += 1
        name = self.t[s:self.p]
        delim = self._getc()
        if delim != 10 and delim >= 0:
            self._line(bytearray())  # the comment
        seq = bytearray()
        while True:
            c = self._getc()
            if c < 0 or c in b">+@":
                break
            if c == 10:
                continue
            seq.append(c)
            self._line(seq)
        if c >= 0 and c in b">@":
            self.pending = True
        if c != ord("+"):
            return name, bytes(seq), None
        while True:
            c = self._getc()
            if c < 0:
                return -2
            if c == 10:
                break
        qual = bytearray()
        while self._line(qual) and len(qual) < len(seq):
            pass
        self.pending = False
        if len(qual) != len(seq):
            return -2
        return name, bytes(seq), bytes(qual)

    def records(self):
        out = []
        while True:
            r = self.read()
            if r is None:
                return out, False
            if r == -2:
                return out, True
            if r[1]:
                out.append(r)


def wrap(s, width):
    return [s[i:i + width] for i in range(0, len(s), width)] if width else [s]


def render(recs, nl=b"\n", width=0, plus_name=False, blanks=(0,), fasta=False, final_nl=True, lead=0, trail=0):
    """recs: (name, seq, qual); blanks: blank lines after record i is blanks[i % len(blanks)]"""
    lines = [b""] * lead
    for i, (name, seq, qual) in enumerate(recs):
        if fasta:
            lines += [b">" + name] + (wrap(seq, width) if seq else [])
        else:
            lines += [b"@" + name] + (wrap(seq, width) if seq or nl == b"\n" else []) + [b"+" + (name.split()[0] if plus_name and name else b"")]
            lines += wrap(qual, width) if qual else [b""]
        lines += [b""] * blanks[i % len(blanks)]
    lines += [b""] * trail
    t = nl.join(lines) + nl
    return t if final_nl else t[:-len(nl)]


def toy_records(n, seed=1, minlen=1, maxlen=150):
    r = random.Random(seed)
    out = []
    for i in range(n):
        ln = r.randint(minlen, maxlen)
        seq = bytes(r.choice(b"ACGTNacgt") for _ in range(ln))
        qual = bytes(r.randint(33, 126) for _ in range(ln))
        out.append((b"r%d/%d some comment" % (i, seed), seq, qual))
    return out


def hand_made():
    """(label, text) pairs: every layout the issue names"""
    recs = toy_records(40, 3)
    recs[5] = (b"@at", b"ACGTACGTACGTACGTACGTA", b"@IIIIII+IIIIII>IIIIII")  # quality lines that start with '@', '+' and '>' when wrapped at 7
    recs[9] = (b"nine", b"ACGTACGTAC", b"+@>+@>+@>+")
    out = [("four-line", render(recs))]
    for w in (7, 20, 33, 1):
        out.append(("wrapped %d" % w, render(recs, width=w, plus_name=True)))
    out.append(("blank lines", render(recs, blanks=(0, 1, 2, 3), lead=2, trail=3)))
    out.append(("wrapped + blank lines", render(recs, width=20, blanks=(1, 0, 3), lead=1, trail=1)))
    out.append(("fasta", render(recs, fasta=True)))
    out.append(("fasta wrapped", render(recs, fasta=True, width=13, blanks=(0, 1), lead=1, trail=2)))
    out.append(("crlf", render(recs, nl=b"\r\n")))
    out.append(("crlf wrapped", render(recs, nl=b"\r\n", width=20, plus_name=True, blanks=(0, 2))))
    out.append(("crlf fasta wrapped", render(recs, nl=b"\r\n", fasta=True, width=20, blanks=(0, 1))))
    out.append(("no final newline", render(recs, width=33, final_nl=False)))
    out.append(("no final newline fasta", render(recs, fasta=True, width=33, final_nl=False)))
    out.append(("no final newline crlf", render(recs, nl=b"\r\n", final_nl=False)))
    empt = list(recs)
    for i in (0, 7, 8, 39):
        empt[i] = (b"empty%d" % i, b"", b"")
    out.append(("empty records", render(empt, width=20, blanks=(0, 1))))
    out.append(("empty records fasta", render(empt, fasta=True, width=20)))
    out.append(("empty lines inside sequences", render(recs, width=9).replace(b"\nA", b"\n\nA")))
    out.append(("fasta with @ markers", render(recs, fasta=True, width=20, blanks=(0, 1)).replace(b">", b"@")))
    out.append(("fastq with > markers", render(recs, width=20).replace(b"\n@r", b"\n>r")))
    out.append(("blank lines of spaces", render(recs, blanks=(1,)).replace(b"\n\n@", b"\n \t \n@")))
    out.append(("only blank lines", b"\n\n  \n\r\n\n"))
    out.append(("empty text", b""))
    out.append(("header only", b"@lonely"))
    # many short records and long wrapped ones: records straddle the boundaries of the tiles the chain is resolved in
    many = toy_records(3000, 5, 1, 9)
    out.append(("many short", render(many, blanks=(0, 0, 1))))
    out.append(("many wrapped 1", render(toy_records(300, 6, 1, 40), width=1)))
    out.append(("one long record", render([(b"long", b"ACGT" * 6000, b"IJKL" * 6000)], width=5) + render(recs)))
    return out


def accepted_text(seed):
    """a text of the class the device ingest must accept, in a random layout"""
    r = random.Random(seed)
    crlf = r.random() < 0.25
    nl = b"\r\n" if crlf else b"\n"
    mode = r.choice(("fastq", "fastq", "fasta", "fasta"))  # (one kind of records per text: a mix may be refused)
    marker = r.choice((None, None, b"@", b">"))  # kseq does not tell the markers apart: '@' FASTA and '>' FASTQ are read as well
    lines = [r.choice((b"", b" ", b"\t ")) if not crlf else b"" for _ in range(r.choice((0, 0, 1, 3)))]
    for i in range(r.randint(0, 30)):
        ln = r.choice((0, 1, 2, 5, 30, 75, 150)) if r.random() < 0.3 else r.randint(1, 120)
        seq = bytes(r.choice(b"ACGTNacgtn") for _ in range(ln))
        # (quality values that look like markers, often at the start of a line)
        qual = bytes(r.choice(b"@+>") if r.random() < 0.15 else r.randint(33, 126) for _ in range(ln))
        name = bytes(r.randint(33, 126) for _ in range(r.randint(0, 12))) + r.choice((b"", b" comment @x", b"\tc"))
        width = r.choice((0, 0, 1, 7, 20, 33, 60))
        fasta = mode == "fasta"
        if crlf and ln == 0 and not fasta:
            continue  # (an empty sequence LINE would be a lone CR: outside the class)
        sl = wrap(seq, width) if seq else ([] if fasta or crlf else r.choice(([], [b""])))
        if len(sl) > 1 and r.random() < 0.2:  # empty lines inside the sequence block (after its first line: a lone CR may not start it)
            k = r.randint(1, len(sl) - 1)
            sl = sl[:k] + [b""] + sl[k:]
        lines += [(marker or (b">" if fasta else b"@")) + name] + sl
        if fasta:
            nb = r.choice((0, 0, 1, 2)) if (seq or not crlf) else 0
            lines += [b""] * nb  # (still the sequence block: empty lines only)
        else:
            lines += [b"+" + r.choice((b"", name.split()[0] if name.split() else b"", b"anything @ here"))]
            lines += wrap(qual, r.choice((width, width, 0, 11))) if qual else [b""]
            lines += [r.choice((b"", b"  ", b"\t")) if not crlf else b"" for _ in range(r.choice((0, 0, 0, 1, 2, 3)))]
    t = nl.join(lines) + nl if lines else b""
    if t and r.random() < 0.3:
        t = t[:-len(nl)]  # (the last line is never a '+' line: a quality line, if only an empty one, follows it)
    return t


def wild_text(seed):
    """an accepted text, damaged: junk lines, lone CRs, qualities cut or lengthened, lines dropped, bytes changed"""
    r = random.Random(seed ^ 0x5eed)
    t = accepted_text(seed)
    lines = t.split(b"\n")
    for _ in range(r.randint(1, 4)):
        if not lines:
            break
        k = r.randrange(len(lines))
        what = r.randrange(8)
        if what == 0:
            lines.insert(k, r.choice((b"junk", b"x @y", b" @late", b"+", b"+x", b"ACGT", b">", b"@")))
        elif what == 1:
            lines.insert(k, b"\r")
        elif what == 2:
            lines[k] = lines[k][:r.randint(0, max(0, len(lines[k]) - 1))]
        elif what == 3:
            lines[k] = lines[k] + bytes(r.randint(33, 126) for _ in range(r.randint(1, 5)))
        elif what == 4:
            del lines[k]
        elif what == 5 and lines[k]:
            b = bytearray(lines[k])
            b[r.randrange(len(b))] = r.choice(b"@+>\r \tAI")
            lines[k] = bytes(b)
        elif what == 6:
            lines[k] = lines[k] + b"\r"
        else:
            lines = lines[:k]
    return b"\n".join(lines)


def expected(text):
    """(names, seqs, quals) lists of the model's records, truncated flag"""
    recs, trunc = Kseq(text).records()
    return [x[0] for x in recs], [x[1] for x in recs], [x[2] for x in recs], trunc
