"""k_s3b_short (the short-list instance of S3b that serves reads of up to 50 bases: lane cap 16) on the device, on hit totals that
straddle its limit: a few thousand 2 x 50 pairs on a genome of 300 kb with planted two- and three-copy segments, so that a read's
~8 minimizers bring 8, 16 or 24 hits and every mixture at a segment's edge.  The totals are counted on the host first
(tests/class_ladder.py's model over the oracle's index) -- 15, 16 and 17 must occur, or the data does not meet the limit.  Mapped with
cmgpu_set_option "s3b_short" 1 and 0: stage trace, list lengths and records equal each other and the oracle.  The same pairs one base
longer equal the oracle too, twice: at default options (the 16-lane groups take the lists beyond 16 hits, which leaves a lane's cap
at 16 for every read length: k_s3b_short on 51-base reads) and with "s3b_lane_cap" 17 (what the read length alone gives: the general
kernel, k_s3b_candidates, whatever the option).  So does one of the repeat-rich fuzz configurations with the option on and with it off."""
import ctypes as C

import numpy as np
import pytest

import class_ladder as cl
import fuzz_data
import oracle_lib as ol
import test_hostemu_fuzz as _fz

pytestmark = pytest.mark.gpu

ACGT, COMP = fuzz_data.ACGT, fuzz_data.COMP
N_PAIRS = 3000
FIELDS = [n for n, _ in ol.OraTrace._fields_]
_CASE = {}


def _pack(rs):
    off = np.zeros(len(rs) + 1, np.uint32)
    off[1:] = np.cumsum([len(r) for r in rs])
    return np.frombuffer(b"".join(rs), np.uint8).copy(), off


def _case(tmp_path_factory):
    """genome, 51-base pairs and their first 50 bases; the oracle's results for both lengths -- once per session"""
    if _CASE:
        return _CASE
    d = tmp_path_factory.mktemp("s3b_short")
    rng = np.random.default_rng(20261019)
    chroms = [ACGT[rng.integers(0, 4, 100_000)].copy() for _ in range(3)]
    segs = []
    for copies, count in ((2, 160), (3, 100)):
        for _ in range(count):
            elem = ACGT[rng.integers(0, 4, 300)]
            for _ in range(copies):
                ci = int(rng.integers(0, 3))
                p = int(rng.integers(500, 100_000 - 800))
                cp = elem.copy()
                m = rng.random(300) < 0.004  # the copies differ in a base or so: some pairs map uniquely, some do not
                cp[m] = ACGT[rng.integers(0, 4, int(m.sum()))]
                chroms[ci][p:p + 300] = cp if rng.random() < 0.5 else COMP[cp[::-1]]
                segs.append((ci, p))
    fa = str(d / "g.fa")
    with open(fa, "wb") as f:
        for i, c in enumerate(chroms):
            f.write(b">c%d\n" % i + c.tobytes() + b"\n")
    r1, r2 = [], []
    for i in range(N_PAIRS):
        fl = int(rng.integers(60, 400))
        if i % 4:  # three pairs in four start in or next to a planted segment
            ci, p = segs[int(rng.integers(0, len(segs)))]
            st = min(max(0, p + int(rng.integers(-60, 300))), 100_000 - fl)
        else:
            ci, st = int(rng.integers(0, 3)), int(rng.integers(0, 100_000 - fl))
        frag = chroms[ci][st:st + fl]
        a, b = frag[:51].copy(), COMP[frag[::-1]][:51].copy()
        for x in (a, b):
            m = rng.random(51) < 0.01
            x[m] = ACGT[rng.integers(0, 4, int(m.sum()))]
        if rng.random() < 0.5:
            a, b = b, a
        r1.append(a.tobytes()); r2.append(b.tobytes())
    kw = {"mapq_threshold": 0}
    o = ol.Oracle(None, fa, ol.params("atac", **kw))
    idx = str(d / "g.idx")
    assert o.L.ora_index_save(idx.encode(), C.byref(o.idx)) == 0
    _CASE.update(fa=fa, idx=idx, kw=kw)
    p = ol.params("atac", **kw)
    ix = cl.IndexLookup(o)
    for L in (50, 51):
        b1, o1 = _pack([r[:L] for r in r1])
        b2, o2 = _pack([r[:L] for r in r2])
        rec, k, st, tr = o.map_pairs(b1, o1, b2, o2, trace=True)
        _CASE[L] = dict(b=(b1, o1, b2, o2), want=_fz._tuples_o(rec, k, False), k=k, st=st.as_dict(),
                        trace=[{f: getattr(tr[i], f) for f in FIELDS} for i in range(N_PAIRS)])
    _CASE["model_tot"] = np.array([cl.model_hit_tot(ix, r[:50], p.max_seed_freq0, p.max_seed_freq1) for pr in zip(r1, r2) for r in pr])
    o.close()
    return _CASE


def _device(g, case, L, label):
    """one mapping of the L-base pairs on the resident context: held to the oracle; returns what two runs are compared by"""
    from chromap_amd import Stats, _capi
    c = case[L]
    st = Stats()
    g.upload(*c["b"])
    k = g.map_resident(st)
    rec, k2 = g.download_records(N_PAIRS)
    assert k2 == k == c["k"], label
    tuples = _fz._tuples_g(rec, k, False)
    assert tuples == c["want"], label
    gst = st.as_dict()
    for key in ("num_candidates", "num_mappings", "num_mapped_reads", "num_uniquely_mapped_reads"):
        assert gst[key] == c["st"][key], (label, key)
    gt = (ol.OraTrace * N_PAIRS)()
    assert g.L.cmgpu_debug_trace(g.ctx, C.cast(gt, C.c_void_p), N_PAIRS) == 0, g.L.cmgpu_last_error(g.ctx)
    trace = [{f: getattr(gt[i], f) for f in FIELDS} for i in range(N_PAIRS)]
    for i in range(N_PAIRS):
        assert trace[i] == c["trace"][i], "%s: pair %d: device %s, oracle %s" % (label, i, trace[i], c["trace"][i])
    arrays = {n: _capi.debug_array(g.L, g.ctx, n, N_PAIRS) for n in ("rlen", "hit_tot", "ncp", "ncn")}
    return tuples, trace, arrays, gst


def test_totals_straddle_the_lane_cap(tmp_path_factory):
    tot = _case(tmp_path_factory)["model_tot"]
    hist = np.bincount(tot, minlength=32)
    print("reads by hit total 0..31:", hist[:32].tolist(), "beyond:", int(hist[32:].sum()))
    for t in (15, 16, 17):
        assert hist[t] > 0, "no read with %d hits" % t
    assert hist[:17].sum() > 1000 and hist[17:].sum() > 1000  # both kernels have work


def test_short_instance_equals_general_kernel_and_oracle(tmp_path_factory):
    from chromap_amd import ChromapGPU
    case = _case(tmp_path_factory)
    g = ChromapGPU(case["idx"], case["fa"], preset="atac", **case["kw"])
    try:
        assert g.get_option("s3b_short") == 1  # the default
        runs = {}
        for on in (1, 0):
            g.set_option("s3b_short", on)
            runs[on] = _device(g, case, 50, "s3b_short = %d" % on)
        for a, b, what in zip(runs[1], runs[0], ("records", "trace", "list lengths", "counters")):
            if what == "list lengths":
                for n in a:
                    assert np.array_equal(a[n], b[n]), n
            else:
                assert a == b, what
        # S3a's totals are the host model's wherever the pair reaches S3a with both reads alive (the device zeroes the others)
        dev = runs[1][2]["hit_tot"][:2 * N_PAIRS]
        full = runs[1][2]["rlen"][:2 * N_PAIRS] == 50  # (the model counts on the read as given: not where the adapter trimming cut it)
        live = (dev > 0) & full
        assert live.sum() > N_PAIRS and np.array_equal(dev[live], case["model_tot"][live])
        assert {15, 16, 17} <= set(int(x) for x in dev[live])
        # one base more, the option on: the short instance again (cap 16 by the size classes), then the general kernel at cap 17
        g.set_option("s3b_short", 1)
        a = _device(g, case, 51, "51-base reads")
        g.set_option("s3b_lane_cap", 17)
        b = _device(g, case, 51, "51-base reads, lane cap 17")
        assert a[0] == b[0] and a[1] == b[1] and a[3] == b[3]
        assert all(np.array_equal(a[2][n], b[2][n]) for n in a[2])
    finally:
        g.close()


@pytest.mark.parametrize("on", [1, 0])
def test_fuzz_configuration_with_the_option_on_and_off(on, tmp_path):
    from chromap_amd import ChromapGPU

    def factory(idx, fa, preset, gkw, b1, o1, b2, o2):
        g = ChromapGPU(idx, fa, preset=preset, **gkw)
        g.set_option("s3b_short", on)
        rec, k = g.map_pairs(b1, o1, b2, o2)
        st = g.stats.as_dict()
        g.close()
        return rec, k, st
    _fz.run_case(factory, fuzz_data.CONFIGS[0], tmp_path)
