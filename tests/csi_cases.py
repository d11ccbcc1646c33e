"""What the CSI index's tests add to the record sets of tests/bai_records.py and the texts of tests/tbi_texts.py: depths other than 5,
positions beyond 2^29, bin numbers beyond 16 bits.  Shared by tests/test_csi_model.py, tests/test_hostemu_csi.py and
tests/test_gpu_csi.py.  Test infrastructure only."""
import bai_model as bai
import bai_records as br
import csi_model as cm
import tbi_texts as tt

DEPTHS = (1, 2, 5, 6)
M1, M3, M10 = ((1, "M"),), ((3, "M"),), ((10, "M"),)

# reference 0's leaf bin is 65536 + X, reference 1's is X: equal keys where the bin has 16 bits of the key (depth 6)
X = cm.level_first(6) + 100
FAR = (65536 + X - cm.level_first(6)) << 14
assert FAR >= 28087 << 14 and cm.reg2bin(FAR, FAR + 5, 6) == 65536 + X and cm.reg2bin(100 << 14, (100 << 14) + 5, 6) == X


def _depth1_records():
    return [br.record(0, 0, M1), br.record(0, 16383, M1), br.record(0, 16383, M3), br.record(0, 16384, M1), br.record(0, 131072 - 10, M10)]


_sets = None


def record_sets():
    """name -> (RecordSet, depth); .refused as in bai_records"""
    global _sets
    if _sets is None:
        s = {}
        s["depth1"] = (br.RecordSet("depth1", 1, _depth1_records(), seams=[(0, 0), (0, 16383), (0, 16384), (0, 16385), (0, 131071)]), 1)
        s["depth1_refused"] = (br.RecordSet("depth1_refused", 1, _depth1_records() + [br.record(0, 131072 - 9, M10)], refused=(bai.RANGE, 6)), 1)
        s["depth2_refused"] = (br.RecordSet("depth2_refused", 1, [br.record(0, (1 << 20) - 10, M10), br.record(0, (1 << 20) - 9, M10)], refused=(bai.RANGE, 2)), 2)
        s["wide_bins"] = (br.RecordSet("wide_bins", 2, [br.record(0, 5), br.record(0, FAR), br.record(0, FAR + 3), br.record(1, 100 << 14), br.record(1, (100 << 14) + 7)],
                                       seams=[(0, 5), (0, FAR), (1, 100 << 14), (0, 100 << 14), (1, FAR)]), 6)
        top = (1 << 31) - 1 - 10
        s["pos_2_31"] = (br.RecordSet("pos_2_31", 1, [br.record(0, 1 << 29, M10), br.record(0, (1 << 30) - 5, M10), br.record(0, top, M10)],
                                      seams=[(0, 1 << 29), (0, 1 << 30), (0, top), (0, top + 10)]), 6)
        # more than one block of the per-record kernels, positions up to 2^31 in steps that change the bin at every level
        n = 2 * br.BLOCK + 3
        s["long_reference_%d" % n] = (br.RecordSet("long_reference_%d" % n, 2, [br.record(i * 2 // n, (i % (n // 2 + 1)) * 4000037, ((70000, "M"),)) for i in range(n)],
                                                   seams=[(0, 4000037 * 100), (1, 4000037 * 200), (0, 1 << 30), (1, 1 << 29)]), 6)
        _sets = s
    return _sets


def regions(rs, depth):
    """bai_records.regions with ends up to the depth's limit"""
    import random
    lim = cm.max_end(depth)
    rnd = random.Random("%s/csi" % rs.name)
    out = []
    for tid, p in rs.seams:
        for q in (p - 1, p, p + 1):
            if q >= 0:
                out += [(tid, q, q + 1), (tid, q, q + 100), (tid, max(0, q - 100), q), (tid, max(0, q - 1), q + 1), (tid, max(0, q - 20000), q + 20000)]
    for _ in range(25):
        tid = rnd.randrange(max(1, rs.n_ref))
        beg = rnd.randrange(lim)
        out.append((tid, beg, beg + rnd.choice((1, 1000, 1 << 20, 1 << 29, lim))))
    out += [(t, 0, lim) for t in range(rs.n_ref)]
    return [(t, b, min(e, lim)) for t, b, e in out if min(e, lim) > b and t < rs.n_ref]


def texts():
    """name -> (text, depth, queries)"""
    rows = tt._rows
    t = {}
    d1 = tt.line(b"chr1", 0, 1) + tt.line(b"chr1", 16383, 16384) + tt.line(b"chr1", 16383, 16386) + tt.line(b"chr1", 16384, 16385) + tt.line(b"chr1", 131000, 131072)
    t["depth1"] = (d1, 1, [(b"chr1", p, p + 1) for p in (0, 16382, 16383, 16384, 16385, 131071)] + [(b"chr1", 0, 131072)])
    far = tt.line(b"chrA", 5, 90) + tt.line(b"chrA", FAR, FAR + 5) + tt.line(b"chrA", FAR + 3, FAR + 9) + tt.line(b"chrB", 100 << 14, (100 << 14) + 5)
    t["wide_bins"] = (far, 6, [(b"chrA", FAR, FAR + 1), (b"chrB", 100 << 14, (100 << 14) + 1), (b"chrA", 100 << 14, (100 << 14) + 1), (b"chrB", FAR, FAR + 1)])
    top = 4294967000
    long_ = rows(b"chr1", 300, first=(1 << 29) - 5000, step=1 << 22, length=5000) + tt.line(b"chr1", top - 300, top) + rows(b"chr2", 300, first=7, step=(1 << 23) + 11, length=1 << 21)
    t["end_4294967000"] = (long_, 6, [(b"chr1", top - 1, top), (b"chr1", top, top + 1), (b"chr1", 1 << 29, (1 << 29) + 1), (b"chr1", (1 << 31) - 7, (1 << 31) + 9),
                                     (b"chr2", 1 << 30, (1 << 30) + (1 << 24)), (b"chr1", 0, 0xffffffff), (b"chr2", 0, 0xffffffff)])
    return t


REFUSED_TEXTS = {
    # name -> (text, depth, 1-based line)
    "depth1_end_131073": (tt.line(b"chr1", 0, 1) + tt.line(b"chr1", 131000, 131073) + tt.line(b"chr1", 131001, 131002), 1, 2),
    "depth6_end_2_32": (tt.line(b"chr1", 0, 1) + tt.line(b"chr1", 4294967000, 4294967296), 6, 2),
    "depth6_start_2_33": (tt.line(b"chr1", 0, 1) + tt.line(b"chr1", 1 << 33, (1 << 33) + 2), 6, 2),
}
