"""The MAPQ stage functions on the device, on their own: cmgpu_debug_mapq (include/chromap_amd_debug.h) runs cm_mapq_single,
cm_mapq_single_split, cm_mapq_paired and cm_mapq_paired_split of chromap_amd/csrc/cm_stages.h -- __dsqrt_rn, the double divisions and
conversions, the narrowing to 8 bits, the two table reads from HBM -- on the cases of tests/mapq_cases.py, one lane per case, and every
byte must equal the plain model's (tests/mapq_model.py).  The context's two tables are downloaded and compared with the host-built ones
bit for bit.  tests/test_mapq_cpu.py holds the model against the oracle, the host build and real records."""
import numpy as np
import pytest

import datasets
import hostemu_valu_lib as hv
import mapq_cases as mc
import oracle_lib as ol

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    from chromap_amd import ChromapGPU
    fa, _, _ = datasets.case_inputs("toy_chip")
    g = ChromapGPU(datasets.case_index("toy_chip"), fa, preset="chip")
    yield g
    g.close()


def device_bytes(g):
    return [g.debug_mapq(x.kind, x.e, x.reads, x.pairs) for x in mc.groups()]


def check_against_model(got):
    for x, (q, tags), dev in zip(mc.groups(), mc.model_results(), got):
        if not np.array_equal(dev, q):  # the other two implementations only for the message
            results = {"device": dev, "model": q, "host": hv.mapq_batch(x.kind, x.e, x.reads, x.pairs),
                       "oracle": ol.mapq_batch(x.kind, x.e, x.reads, x.pairs)}
            pytest.fail(mc.first_difference(x, tags, results))


def check_tables(g):
    coef, brk = g.debug_mapq_tables()
    hcoef, hbrk = hv.mapq_tables()
    assert brk.dtype == hbrk.dtype and np.array_equal(brk, hbrk)
    assert coef.shape == (65536,) and np.array_equal(coef.view(np.uint64), hcoef.view(np.uint64))


def test_resident_tables_equal_the_host_built_ones(gpu):
    check_tables(gpu)


def test_device_mapq_equals_the_model_on_every_case(gpu):
    got = device_bytes(gpu)
    assert sum(len(d) for d in got) == sum(x.pairs.shape[1] for x in mc.groups())
    check_against_model(got)


def test_mapping_does_not_disturb_the_tables(gpu):
    before = device_bytes(gpu)
    _, r1, r2 = datasets.case_inputs("toy_chip")
    b1, o1 = ol.read_fastx(r1)
    b2, o2 = ol.read_fastx(r2)
    _, k = gpu.map_pairs(b1, o1, b2, o2)
    assert k > 0
    check_tables(gpu)
    after = device_bytes(gpu)
    for x, a, b in zip(mc.groups(), before, after):
        assert np.array_equal(a, b), x.name
    check_against_model(after)


def test_hook_rejects_bad_arguments(gpu):
    x = mc.groups()[0]
    with pytest.raises(ValueError):
        gpu.debug_mapq(x.kind, x.e, x.reads[:, :-2], x.pairs)
    with pytest.raises(RuntimeError):
        gpu.debug_mapq(7, x.e, x.reads[:, :2], x.pairs[:, :1])
    assert len(gpu.debug_mapq(x.kind, x.e, x.reads[:, :0], x.pairs[:, :0])) == 0
