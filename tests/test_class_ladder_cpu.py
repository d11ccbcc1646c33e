"""The class ladder (tests/class_ladder.py) held to its plan before any GPU sees it: for every tier, the lengths the generator
planned are what the oracle's trace and a plain Python model of the hit and rescue-hit counts give, and every boundary of the
size-class table that the tier names is met exactly at B - 1, B and B + 1 (rescue lengths are products: where a length does not
factor, the nearest one the reads can give, listed in `unmet`).  The smallest tiers also run through the stage functions'
host build with the real geometry of the classes they meet."""
import ctypes as C

import pytest

import class_ladder as cl
import oracle_lib as ol

_RESULT = {}


def oracle_result(name):
    """(case, records as sorted tuples, k, counters, trace, model lengths) of a tier, computed once and left unchanged"""
    if name not in _RESULT:
        from test_hostemu_fuzz import _tuples_o
        case = cl.get_case(name)
        o = cl.oracle_for(case)
        rec, k, st, tr = o.map_pairs(case.b1, case.o1, case.b2, case.o2, trace=True)
        trace = [{f: getattr(tr[i], f) for f, _ in ol.OraTrace._fields_} for i in range(case.n_pairs)]
        model = cl.model_lengths(case, o)
        _RESULT[name] = (case, _tuples_o(rec, k, False), k, st.as_dict(), trace, model)
        o.close()
    return _RESULT[name]


@pytest.mark.parametrize("name", list(cl.TIERS))
def test_plan_holds_in_oracle_and_model(name):
    case, _, k, st, trace, model = oracle_result(name)
    print("%s: genome %d bases, %d pairs, %d planned lengths, %d records" % (name, case.genome, case.n_pairs, len(case.plan), k))
    # the oracle's trace: candidates, draft mappings and co-best pairings of the planned pairs
    for i, want in case.trace.items():
        for f, v in want.items():
            if f == "rep2_nonzero":
                assert trace[i]["rep2"] > 0, (name, i, "read 2 has no repetitive-seed length")
            else:
                assert trace[i][f] == v, (name, i, f, trace[i][f], v)
    seen = {}
    for n, e in enumerate(case.plan):
        t = trace[e["pair"]]
        if e["kind"] in ("hit", "rescue"):  # the two lengths the trace does not carry: the model
            assert model[n] == e["want"], (name, e["pair"], e["array"], model[n], e["want"])
        elif e["kind"] == "nbest":
            assert t["nbest"] == e["want"], (name, e["pair"], t["nbest"], e["want"])
        else:  # per-strand candidate / draft lists: the trace carries their sums per read (held to case.trace above), the
            # generator the split -- the copies it planted on each strand
            fam = case.families[e["fam"]]
            assert sum(b["strand"] == 0 for b in fam["copies"]) == fam["cp"] and len(fam["copies"]) == fam["cp"] + fam["cn"]
            m = "1" if e["mate"] == 0 else "2"
            assert t["n_cand" + m] == fam["cp"] + fam["cn"] == t["n_draft" + m], (name, e["pair"], e["array"])
        seen.setdefault((e["array"], e["boundary"]), set()).add(e["want"])
    # coverage is a condition: every boundary of the tier at B - 1, B and B + 1, in every array it applies to
    unmet = {(u["boundary"], u["want"]): u for u in case.unmet}
    for arrays, B, length in cl.required_lengths(name):
        got = set().union(*(seen.get((a, B), set()) for a in arrays))
        if (B, length) in unmet:
            assert arrays == ("resc_p", "resc_n"), "only a rescue length may be met to the nearest attainable one"
            assert unmet[(B, length)]["nearest"] in got
        else:
            assert length in got, (name, arrays, B, length, sorted(got))
    for u in case.unmet:
        print("%s: rescue boundary %d: length %d is no product the reads offer, nearest %d" % (name, u["boundary"], u["want"], u["nearest"]))
    assert all(u["array"] == "resc_p/resc_n" for u in case.unmet)


def test_every_boundary_of_the_table_is_in_some_tier():
    tiers = cl.TIERS.values()
    assert {b for t in tiers for b in t[1] if t[0] == 50} == set(cl.HIT_B[50])
    assert {b for t in tiers for b in t[1] if t[0] == 100} == set(cl.HIT_B[100])
    assert {b for t in tiers for b in t[2]} == set(cl.CAND_B)
    assert {b for t in tiers for b in t[3]} == set(cl.NBEST_B)
    assert {b for t in tiers for b in t[4]} == set(cl.RESCUE_B) >= {3968, 7680}


# the classes the small tiers meet, as tests/hostemu takes them: (group size, list length above which a read goes to a group, entries
# of the class's work area = the default P of the class, minimizer table, run table)
HOSTEMU_GEOMETRIES = {
    "lane_50": [(16, 16, 64, 64, 130), (64, 16, 256, 64, 130), (64, 16, 512, 64, 130)],   # hv_mid, hv_sub, hv_max[0]
    "lane_100": [(16, 16, 96, 64, 130)],                                                 # hv_mid of reads of 100 bases and more
}


@pytest.mark.parametrize("name,geo", [(n, g) for n, gs in HOSTEMU_GEOMETRIES.items() for g in gs],
                         ids=["%s-G%d_P%d" % (n, g[0], g[2]) for n, gs in HOSTEMU_GEOMETRIES.items() for g in gs])
def test_small_tiers_through_the_stage_functions(name, geo):
    import hostemu_lib as he
    from test_hostemu_fuzz import CAPI_NAMES, _tuples_g
    case, want, k, st, _, _ = oracle_result(name)
    L = he.lib()
    h = he.HostEmu(case.idx, case.fa, he.params(case.preset, **{CAPI_NAMES.get(a, a): v for a, v in case.kw.items()}))
    L.hostemu_set_coop.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
    L.hostemu_set_coop(*geo)
    try:
        rec, gk, gst, _ = h.map_pairs(case.b1, case.o1, case.b2, case.o2)
        items = (C.c_ulonglong * 12)()
        L.hostemu_coop_items(items)
    finally:
        L.hostemu_set_coop(0, 0, 0, 0, 0)
    assert gk == k and _tuples_g(rec, gk, False) == want
    gs = gst.as_dict()
    for key in ("num_candidates", "num_mappings", "num_mapped_reads", "num_uniquely_mapped_reads"):
        assert gs[key] == st[key], key
    assert items[0] > 0, "no read went through the cooperative hit-list stage"
