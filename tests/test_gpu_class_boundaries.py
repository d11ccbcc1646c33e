"""The long-list size classes at the sizes the library ships with (the table at the top of chromap_amd/csrc/cm_types.h): every tier
of tests/class_ladder.py is mapped at DEFAULT options -- no cmgpu_set_option call touches a class -- and held to the oracle:
records, counters, the stage trace pair by pair, the list lengths the plan names (cmgpu_debug_array; for hit_tot and the rescue
hits against the Python model of tests/class_ladder.py), and the class every planned list belongs to had items ("hv_cnt").
tests/test_class_ladder_cpu.py proves on the CPU that the plan meets every boundary at B - 1, B and B + 1."""
import ctypes as C
import time

import numpy as np
import pytest

import class_ladder as cl
import oracle_lib as ol
from test_class_ladder_cpu import oracle_result
from test_hostemu_classes import classes

pytestmark = pytest.mark.gpu

from class_ladder import (COOP_MIN, HIT_B256A, HIT_B256B, HIT_B512, HIT_B1024, HIT_DECLINED, HIT_G16, HIT_SERIAL, HIT_SLAB, HIT_WAVE,  # noqa: E402
                          HIT_WAVE_SMALL, PF_BLOCK, PF_BLOCK_BIG, PF_HUGE, PF_WAVE, RS_B256A, RS_B256B, RS_B512, RS_B1024, RS_SLAB, RS_WAVE,
                          S5_BLOCK, S5_SMALL, S5_WAVE, S6A_BLOCK, S6A_LISTS, S6A_SMALL, S6A_WAVE, S6C_BLOCK, S6C_LISTS, S6C_MULTI, S6C_SMALL,
                          S6C_WAVE, SLAB_CAP, _hit_class, _pf_class, _rescue_class, _s5_class, _s6_class)
# list ids that cannot have items in these cases, and why
NEVER = {HIT_DECLINED: "k_s3b_coop declines a read only when a hit's diagonal lies before its sequence's start or its run table overflows: "
                       "the ladder's copies stand clear of the chromosome ends (tests/test_gpu_stages.py has the wrapped diagonal)"}
FIELDS = [n for n, _ in ol.OraTrace._fields_]
STAGE_OF = {"len": "K0 trimming", "n_mm": "K1 minimizers", "n_cand": "K2/K3 probe, candidates, rescue, pair filter", "rep": "K3 repetitive seeds",
            "n_draft": "K4 verification", "min_err": "K4 verification", "nbest": "K4/K5 best mappings", "second": "K4 verification",
            "nsecond": "K4 verification", "min_sum": "K5 pairing", "second_sum": "K5 pairing", "force_mapq": "K3c supplement"}
ARRAYS = ("hit_tot", "ncp", "ncn", "resc_p", "resc_n", "mcp", "mcn", "fcp", "fcn", "ndp", "ndn", "nv", "pe_nbest")
_SEEN = {}    # tier -> list ids that had items in its default run


def _context(case):
    from chromap_amd import ChromapGPU
    from test_hostemu_fuzz import CAPI_NAMES
    oracle_result(case.name)  # (writes the index file)
    return ChromapGPU(case.idx, case.fa, preset=case.preset, **{CAPI_NAMES.get(k, k): v for k, v in case.kw.items()})


def _map(g, case):
    """one mapping call on the resident context: (sorted record tuples, k, counters)"""
    from chromap_amd import Stats
    from test_hostemu_fuzz import _tuples_g
    st = Stats()
    g.upload(case.b1, case.o1, case.b2, case.o2)
    k = g.map_resident(st)
    rec, k2 = g.download_records(max(1, case.n_pairs))
    assert k2 == k
    return _tuples_g(rec, k, False), k, st.as_dict()


def _arrays(g, case):
    from chromap_amd import _capi
    a = {n: _capi.debug_array(g.L, g.ctx, n, case.n_pairs).astype(np.int64) for n in ARRAYS}
    a["hv_cnt"] = _capi.debug_array(g.L, g.ctx, _capi.DEBUG_LIST_COUNTERS, case.n_pairs).astype(np.int64)[:_capi.HV_LISTS]
    return a


def _compare(case, got, label):
    """records, counters of one device run against the oracle's"""
    _, want, k, st, _, _ = oracle_result(case.name)
    tuples, gk, gst = got
    assert gk == k, label
    assert tuples == want, label
    for key in ("num_candidates", "num_mappings", "num_mapped_reads", "num_uniquely_mapped_reads"):
        assert gst[key] == st[key], (label, key)


def _compare_trace(g, case, label):
    trace = oracle_result(case.name)[4]
    n = case.n_pairs
    gt = (ol.OraTrace * n)()  # cmgpu_trace has ora_trace's layout
    assert g.L.cmgpu_debug_trace(g.ctx, C.cast(gt, C.c_void_p), n) == 0, g.L.cmgpu_last_error(g.ctx)
    for i in range(n):
        for f in FIELDS:
            if getattr(gt[i], f) != trace[i][f]:
                stage = next(v for p, v in STAGE_OF.items() if f.startswith(p))
                raise AssertionError("%s pair %d: %s = %d on the device, %d in the oracle (stage: %s)" % (label, i, f, getattr(gt[i], f), trace[i][f], stage))


def _expected_lists(case, arrays, cls):
    """list id -> the planned (pair, array, length) that must have put an item there"""
    out = {}
    for e in case.plan:
        i = e["pair"]
        why = (i, e["array"], e["want"])
        if e["kind"] == "hit":
            lid = _hit_class(e["want"], cls)
            if lid is not None:
                out.setdefault(lid, why)
            if e["want"] > SLAB_CAP:
                out.setdefault(HIT_SERIAL, why)  # the slab launch declines what its slab does not hold: one lane
        elif e["kind"] == "rescue":
            r = 2 * i + e["mate"]
            lid = _rescue_class(max(int(arrays["resc_p"][r]), int(arrays["resc_n"][r])), cls)
            assert lid is not None
            out.setdefault(lid, why)
        elif e["kind"] == "cand" and e["array"] in ("mcp", "mcn", "fcp", "fcn", "ndp", "ndn"):
            fam = case.families[e["fam"]]
            big = max(fam["cp"], fam["cn"])  # every read of the pair has one list of that length and one of the other
            if e["want"] != big or big <= COOP_MIN:
                continue
            if e["array"][0] == "m":
                lid = _pf_class(big)
                if lid is not None:
                    out.setdefault(lid, why)
            elif e["array"][0] == "f":
                out.setdefault(_s5_class(big, 0), why)
            else:
                q = _s6_class(big, big)
                out.setdefault(S6A_LISTS[q], why)
                out.setdefault(S6C_LISTS[q], why)  # cp + cn co-best pairings: a multi-mapped pair
                out.setdefault(S6C_MULTI, why)
    return out


def _expected_counts(case, arrays, cls):
    """list id -> items, for the lists whose class follows from the downloaded lengths alone"""
    from collections import Counter
    out = Counter({l: 0 for l in (HIT_G16, HIT_WAVE_SMALL, HIT_WAVE, HIT_B256A, HIT_B256B, HIT_B512, HIT_B1024, HIT_SLAB, RS_B256A, RS_B256B, RS_B512,
                                  RS_B1024, RS_SLAB, PF_WAVE, PF_BLOCK, PF_BLOCK_BIG, PF_HUGE, S5_SMALL, S5_WAVE, S5_BLOCK, S6A_SMALL, S6A_WAVE,
                                  S6A_BLOCK, S6C_SMALL, S6C_WAVE, S6C_BLOCK, S6C_MULTI)})
    for tot in arrays["hit_tot"]:  # S3a lists every read by its hit count
        lid = _hit_class(int(tot), cls)
        if lid is not None:
            out[lid] += 1
    # rescue hits: the planned reads are the only ones with more than RS_COOP_MIN of them (list 6 also takes reads whose lists are only copied)
    for r in sorted({2 * e["pair"] + e["mate"] for e in case.plan if e["kind"] == "rescue"}):
        lid = _rescue_class(max(int(arrays["resc_p"][r]), int(arrays["resc_n"][r])), cls)
        if lid != RS_WAVE:
            out[lid] += 1
    a = {n: arrays[n].reshape(-1, 2) for n in ("mcp", "mcn", "fcp", "fcn", "ndp", "ndn")}  # [pair, mate]
    for i in range(case.n_pairs):
        m = [int(a["mcp"][i, 0]), int(a["mcn"][i, 0]), int(a["mcp"][i, 1]), int(a["mcn"][i, 1])]
        if m[0] + m[1] == 0 or m[2] + m[3] == 0:
            continue  # a pair one of whose reads has no candidate ends before the pair filter
        lid = _pf_class(max(m))
        if lid is not None:
            out[lid] += 1
        f = [int(a["fcp"][i, 0]), int(a["fcn"][i, 0]), int(a["fcp"][i, 1]), int(a["fcn"][i, 1])]
        if f[0] + f[1] == 0 or f[2] + f[3] == 0:
            continue
        for p_, n_ in ((f[0], f[1]), (f[2], f[3])):
            if _s5_class(p_, n_) is not None:
                out[_s5_class(p_, n_)] += 1
        d = [int(a["ndp"][i, 0]), int(a["ndn"][i, 0]), int(a["ndp"][i, 1]), int(a["ndn"][i, 1])]
        if d[0] + d[1] == 0 or d[2] + d[3] == 0:
            continue
        q = _s6_class(max(d), max(d[2], d[3]))  # the class by read 2's longer list
        if q is not None:
            out[S6A_LISTS[q]] += 1
        if q is not None or arrays["pe_nbest"][i] > 1:
            out[S6C_MULTI] += 1
        if q is not None and arrays["pe_nbest"][i] > 1:
            out[S6C_LISTS[q]] += 1
    return out


def _check_lengths_and_classes(g, case, label, goff=True):
    arrays = _arrays(g, case)
    model = oracle_result(case.name)[5]
    for n, e in enumerate(case.plan):
        i = e["pair"] if e["mate"] is None else 2 * e["pair"] + e["mate"]
        got = int(arrays[e["array"]][i])
        if n in model:  # hit_tot and the rescue hits: the Python model's count, which the CPU test holds to the plan
            assert got == model[n] == e["want"], "%s pair %d: %s = %d on the device, %d in the model, %d planned" % (label, e["pair"], e["array"], got, model[n], e["want"])
        else:
            assert got == e["want"], "%s pair %d mate %s: %s = %d on the device, %d planned" % (label, e["pair"], e["mate"], e["array"], got, e["want"])
    cls = classes(max_read_len=case.max_read_len, n_seq=3, goff=goff)
    hv = arrays["hv_cnt"]
    print("%s: classes %s" % (label, cls))
    print("%s: items per list id %s" % (label, {l: int(hv[l]) for l in range(32) if hv[l]}))
    for lid, why in sorted(_expected_lists(case, arrays, cls).items()):
        assert hv[lid] > 0, "%s: list %d had no item, although pair %d has %s = %d" % (label, lid, why[0], why[1], why[2])
    # where a list's class is a function of one downloaded length, every list has exactly the reads of its class: one entry too
    # many or too few at a boundary shows here even when the neighbouring class computes the same result
    want = _expected_counts(case, arrays, cls)
    print("%s: expected items per list id %s" % (label, {l: n for l, n in sorted(want.items()) if n}))
    bad = ["list %d has %d items, the lengths put %d reads / pairs in its class" % (lid, hv[lid], n) for lid, n in sorted(want.items()) if hv[lid] != n]
    assert not bad, "%s: %s" % (label, "; ".join(bad))
    return {l for l in range(32) if hv[l] > 0}


def device_run(name):
    """the tier on a fresh context at default options, once per session: the list ids that had items"""
    if name not in _SEEN:
        case = cl.get_case(name)
        t0 = time.time()
        oracle_result(name)
        t1 = time.time()
        g = _context(case)
        t2 = time.time()
        got = _map(g, case)
        t3 = time.time()
        print("%s: oracle (generator, index, mapping, model) %.1f s, device context %.1f s, upload + mapping + download %.2f s" % (name, t1 - t0, t2 - t1, t3 - t2))
        try:
            _compare(case, got, name)
            _compare_trace(g, case, name)
            _SEEN[name] = _check_lengths_and_classes(g, case, name)
        finally:
            g.close()
    return _SEEN[name]


@pytest.mark.parametrize("name", list(cl.TIERS))
def test_tier_at_default_options(name):
    device_run(name)


def test_every_list_id_had_items_in_some_tier():
    seen = set().union(*(device_run(name) for name in cl.TIERS))
    missing = sorted(set(range(32)) - seen - set(NEVER))
    assert not missing, "no tier put an item on list(s) %s" % missing
    assert not (seen & set(NEVER)), "a list named as impossible had items: %s" % sorted(seen & set(NEVER))


def test_range_mapped_again_when_a_class_was_not_launched():
    """The speculative launch set: a context launches the kernels of the classes that had items lately (a fresh one: of every
    class).  A batch without long lists empties the set; the tier that follows finds items in classes it did not launch for and is
    mapped again with every class on; the same tier once more is mapped with no re-run.  Both give the oracle's records."""
    case = cl.get_case("block_1k_2k")
    g = _context(case)
    try:
        short = [i for i, t in case.trace.items() if t.get("nbest") == 1][:8]  # the uniquely mapping pairs

        def sub(b, o):
            parts = [b[o[i]:o[i + 1]] for i in short]
            off = np.zeros(len(parts) + 1, np.uint32)
            off[1:] = np.cumsum([len(p) for p in parts])
            return np.concatenate(parts), off
        b1, o1 = sub(case.b1, case.o1)
        b2, o2 = sub(case.b2, case.o2)
        g.upload(b1, o1, b2, o2)
        assert g.map_resident() == len(short)
        from chromap_amd import _capi
        hv = _capi.debug_array(g.L, g.ctx, _capi.DEBUG_LIST_COUNTERS, len(short))[:32]
        assert hv[6:].sum() == 0, "the priming batch has long lists"
        first = _map(g, case)
        _compare(case, first, "after a batch without long lists")
        _compare_trace(g, case, "after a batch without long lists")
        assert _check_lengths_and_classes(g, case, "after a batch without long lists") & set(range(6, 32)), "no class had items: nothing was mapped again"
        second = _map(g, case)
        _compare(case, second, "second call")
        assert first == second
    finally:
        g.close()


def test_largest_hit_class_on_64_bit_keys(monkeypatch):
    """64-bit hit keys (a reference too long for 32-bit global coordinates gets these; CM_NO_KEY32 asks for them on any): the
    largest hit-list class holds 8192 hits instead of 7040"""
    monkeypatch.setenv("CM_NO_KEY32", "1")
    case = cl.get_case(cl.HIT_KEY64_TIER)
    g = _context(case)
    try:
        _compare(case, _map(g, case), "64-bit keys")
        _compare_trace(g, case, "64-bit keys")
        seen = _check_lengths_and_classes(g, case, "64-bit keys", goff=False)
        assert classes(max_read_len=case.max_read_len, n_seq=3, goff=False)["hv_big"] == 8192
        assert {HIT_B1024, HIT_SLAB} <= seen
    finally:
        g.close()


@pytest.mark.parametrize("option,value", [("heavy_wave_max", -1), ("coop", 0)])
def test_classes_decide_who_works_never_the_result(option, value):
    """cm_classes.h's sentence at real sizes: the tier with every long list on the one-lane path / with no stage's lists given to
    groups gives the records of the default run (which equal the oracle's)"""
    case = cl.get_case("block_1k_2k")
    device_run(case.name)
    g = _context(case)
    try:
        g.set_option(option, value)
        _compare(case, _map(g, case), "%s = %d" % (option, value))
        _compare_trace(g, case, "%s = %d" % (option, value))
    finally:
        g.close()
