"""The CPU oracle against the REAL reference on parameter frames outside the editor's ranges (tests/domain_cases.py,
vectors in tests/golden/vtm_domain_golden.npz): the double and the float restatement reproduce every vector bit for bit,
so that tests/test_gpu_domain.py may hold the kernels to the oracle there.

Reference model 5 has a table and a module of its own: tests/domain5_cases.py, tests/test_domain5_cpu.py."""
import functools

import numpy as np
import pytest

import domain_cases
import oracle


@functools.lru_cache(maxsize=None)
def golden():
    data = domain_cases.golden()
    for k, v in data.items():
        if k != "manifest":
            v.setflags(write=False)
    return data


@pytest.mark.parametrize("cls", domain_cases.CLASSES, ids=[domain_cases.class_key(c) for c in domain_cases.CLASSES])
def test_oracle_reproduces_the_reference_bit_for_bit(cls):
    model, delay, layout, fm = cls
    data = golden()
    fs = domain_cases.class_fs(data["manifest"], cls)
    cfg = oracle.male_config(domain_cases.RATE, delay, layout, float_model=fm)
    assert float(oracle.derive(cfg).sample_rate) == fs
    outs = oracle.synthesize_many([(domain_cases.track_for(c, fs), domain_cases.RATE, delay, layout, fm) for c in domain_cases.CASES])
    for case, out in zip(domain_cases.CASES, outs):
        domain_cases.check_against_golden(out, case, cls, data)


def test_every_vector_is_finite_and_audible():
    data = golden()
    assert len(data) - 1 == len(domain_cases.CASES) * len(domain_cases.CLASSES) == len(data["manifest"])
    for cls in domain_cases.CLASSES:
        for case in domain_cases.CASES:
            k = domain_cases.key(case, cls)
            v, m = data[k], data["manifest"][k]
            assert v.dtype == np.float32 and v.size == m["n"] and m["fs"] == domain_cases.class_fs(data["manifest"], cls), k
            assert np.isfinite(v).all() and np.abs(v).max() == m["peak"] > 0.0, k


@pytest.mark.parametrize("cls", domain_cases.CLASSES, ids=[domain_cases.class_key(c) for c in domain_cases.CLASSES])
def test_the_family_tells_the_tap_branches_apart(cls):
    """A position in (-2, -1) injects nothing, -1.0 likewise but by another branch, (-1, 0) all of it into the first
    section: the -1.5 vector differs from the -1.0 one (the track passes through (-1, 0) on its way to either, where -1.5
    has other shares), and both from -0.5."""
    data = golden()
    a, b, c = (data[domain_cases.key(domain_cases.BY_NAME[n], cls)] for n in ("fpos_m1.5", "fpos_m1", "fpos_m0.5"))
    assert a.size == b.size == c.size
    assert not np.array_equal(a, b) and not np.array_equal(a, c) and not np.array_equal(b, c)


def test_float_pinned_flags_are_what_the_tracks_say():
    """A case's flag = every float conversion argument of its track inside the pinned ranges, at the internal rate of every class."""
    manifest = golden()["manifest"]
    rates = sorted({domain_cases.class_fs(manifest, cls) for cls in domain_cases.CLASSES})
    assert rates == [20034.0, 40068.0, 60102.0]  # 10 + 6 tube, the same at SectionDelay 2, 30 + 18 tube
    for case in domain_cases.CASES:
        per_rate = [domain_cases.float_pinned(domain_cases.track_for(case, fs), fs) for fs in rates]
        assert case["float_pinned"] == all(per_rate), (case["name"], per_rate)
    unpinned = [c["name"] for c in domain_cases.CASES if not c["float_pinned"]]
    assert unpinned == ["fcf_60k", "fcf_9e5", "fbw_0.45fs", "fbw_0.49fs", "fbw_0.5fs"]
    # the 30 + 18 tube's rate brings 60 kHz back inside cosf's range (6.3 rad): pinned there
    assert domain_cases.float_pinned(domain_cases.track_for(domain_cases.BY_NAME["fcf_60k"], 60102.0), 60102.0)
    assert len({c["name"] for c in domain_cases.CASES}) == len(domain_cases.CASES)
    # a bar of its own only where the arguments leave the pinned ranges, and only the one measured case has one
    assert [c["name"] for c in domain_cases.CASES if c["float_bar"] is not None] == ["fcf_9e5"]
    assert not domain_cases.BY_NAME["fcf_9e5"]["float_pinned"] and domain_cases.BY_NAME["fcf_9e5"]["float_bar"] == 4 * 2.02e-5
