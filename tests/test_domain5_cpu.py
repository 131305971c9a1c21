"""The CPU oracle of reference model 5 against the REAL reference on parameter frames outside the editor's ranges
(tests/domain5_cases.py, vectors in tests/golden/vtm5_domain_golden.npz): the double and the float restatement reproduce
every vector bit for bit, so that tests/test_gpu_domain5.py may hold the kernels to the oracle there -- frication positions
down to S1 and up to S30 included, which the reference computes as plain C++.

Where the position's section lies outside S1..S30 the reference indexes out of bounds and has no vector; there the oracle
follows the product's rule (nothing is injected, decided on the floating offset), which is pinned here as "the same frames
with fricVol 0"."""
import numpy as np
import pytest

import domain5_cases as cases
import domain_cases
import oracle
from gama_tts_amd import capi
from parity_rules import TOL
from voice_cases import model5_plan

CLASS_IDS = [cases.class_key(c) for c in cases.CLASSES]


@pytest.mark.parametrize("cls", cases.CLASSES, ids=CLASS_IDS)
def test_oracle_reproduces_the_reference_bit_for_bit(cls):
    data = cases.golden()
    todo = [v for v in cases.vector_keys() if v[2] == cls]
    outs = cases.synthesize_many([(config, cls[1], cases.track_for(case)) for case, config, _ in todo])
    assert len(todo) == len(data["manifest"]) // 2
    for (case, config, _), out in zip(todo, outs):
        cases.check_against_golden(out, case, config, cls, data)


def test_every_vector_is_finite_and_audible():
    data = cases.golden()
    keys = [cases.key(*v) for v in cases.vector_keys()]
    assert len(set(keys)) == len(keys) == len(data) - 1 == len(data["manifest"]) and set(keys) == set(data["manifest"])
    assert len({c["name"] for c in cases.CASES}) == len(cases.CASES)
    for case, config, cls in cases.vector_keys():
        k = cases.key(case, config, cls)
        v, m = data[k], data["manifest"][k]
        assert v.dtype == np.float32 and v.size == m["n"], k
        assert np.isfinite(v).all() and np.abs(v).max() == m["peak"] > 0.0, k
    # every male-voice configuration runs at MALE_FS, the lowest rate of all (the reference reports it in float)
    for case, config, cls in cases.vector_keys():
        fs = data["manifest"][cases.key(case, config, cls)]["fs"]
        if cases.CONFIGS[config][0] == "male":
            assert abs(fs - cases.MALE_FS) < 4e-3, (config, fs)
        else:
            assert fs > cases.MALE_FS
    # the band-pass that grows: still finite, far above every other vector
    assert data["manifest"]["fbw_m500__male__m5"]["peak"] > 1e11


def test_the_table_has_no_vector_for_the_product_rule_cases():
    manifest = cases.golden()["manifest"]
    assert len(cases.PRODUCT_CASES) == 9 and all(c["base"] == "F" and c["configs"] == ("male",) for c in cases.PRODUCT_CASES)
    assert not [k for k in manifest if k.startswith("prod_")]
    for c in cases.PRODUCT_CASES:
        t = cases.track_for(c)
        last = [cases.section_index(t[-1, 4], dt) for dt in (np.float32, np.float64)]
        assert not 0 <= last[0] <= 29 and not 0 <= last[1] <= 29, (c["name"], last)
        if c["form"] == "const":
            assert (t == t[0]).all()
        else:
            assert np.array_equal(t[0], cases.base_frame("F")) and (np.diff(t[:, 4]) != 0).all()


def test_positions_land_in_the_sections_the_table_names():
    """5 + trunc(22 * pos / 7), formed in float and in double as the two classes form it, is the table's section; both
    ends of the tube (S1 = 0, S30 = 29) and their inner neighbours are there, on both bases."""
    seen = set()
    for case in cases.REFERENCE_CASES:
        if case["section"] is None:
            assert 4 not in case["overrides"], case["name"]
            continue
        pos = case["overrides"][4]
        assert cases.section_index(pos, np.float32) == cases.section_index(pos, np.float64) == case["section"], case["name"]
        assert 0 <= case["section"] <= 29
        seen.add((case["section"], case["base"]))
    for section in (0, 1, 4, 5, 27, 28, 29):
        assert (section, "B") in seen and (section, "F") in seen, section
    # the base's own position is inside the editor's range
    assert 0.0 <= cases.base_frame("B")[4] <= 7.0 and cases.base_frame("F")[4] == cases.base_frame("B")[4]
    assert cases.base_frame("F")[1:4].tolist() == [0.0, 0.0, 60.0]


@pytest.mark.parametrize("cls", cases.CLASSES, ids=CLASS_IDS)
@pytest.mark.parametrize("base", ["B", "F"])
def test_the_family_tells_the_edge_sections_apart(cls, base):
    """S1 (-1.7), S2 (-1.5), S29 (7.5) and S30 (7.8): pairwise different vectors."""
    data = cases.golden()
    vs = [data[cases.key(cases.BY_NAME["fpos_%s_%s" % (n, base)], "male", cls)] for n in ("m1.7", "m1.5", "7.5", "7.8")]
    assert [cases.BY_NAME["fpos_%s_%s" % (n, base)]["section"] for n in ("m1.7", "m1.5", "7.5", "7.8")] == [0, 1, 28, 29]
    for i in range(4):
        for j in range(i):
            assert vs[i].size == vs[j].size and not np.array_equal(vs[i], vs[j]), (i, j)


def test_float_pinned_flags_are_what_the_tracks_say():
    """A case's flag = every float conversion argument of its track inside the pinned ranges, at the internal rate of every
    configuration that makes it."""
    manifest = cases.golden()["manifest"]
    f = cases.CLASSES[1]
    for case in cases.REFERENCE_CASES:
        per = [cases.float_pinned5(cases.track_for(case), manifest[cases.key(case, cfg, f)]["fs"]) for cfg in case["configs"]]
        assert case["float_pinned"] == all(per), (case["name"], per)
        if not case["float_pinned"]:
            assert not any(per), (case["name"], per)  # (outside at EVERY voice's rate: one rule per case)
    for case in cases.PRODUCT_CASES:
        assert case["float_pinned"] and cases.float_pinned5(cases.track_for(case), cases.MALE_FS), case["name"]
    assert [c["name"] for c in cases.CASES if not c["float_pinned"]] == ["fcf_9e5", "fbw_0.45fs", "fbw_0.49fs"]
    assert cases.float_pinned5 is not domain_cases.float_pinned and domain_cases.PINNED["tan"] == 1.38
    # a bar of its own only for a case that cannot be bit-identical, with its reason in the table: the tracks that enter
    # S1, whose share the kernel folds into the tube input, at the mixed path's bar
    barred = [c["name"] for c in cases.CASES if c["float_bar"] is not None]
    assert barred == list(cases.FLOAT_BAR_REASONS) and cases.S1_FLOAT_BAR == TOL[capi.PRECISION_MIXED]
    for c in cases.CASES:
        pos = cases.track_for(c)[:, 4].astype(np.float64)  # (every step of the interpolation between two frames)
        steps = np.concatenate([np.linspace(a, b, 243) for a, b in zip(pos[:-1], pos[1:])])
        sections = {cases.section_index(p, np.float32) for p in steps if abs(p) < 1e6}
        assert (c["float_bar"] == cases.S1_FLOAT_BAR) == (0 in sections) and c["float_bar"] in (None, cases.S1_FLOAT_BAR), c["name"]
    # bandwidth cases never exceed half of any voice's rate
    for c in cases.CASES:
        if c["bw_factor"] is not None:
            assert 0.0 < c["bw_factor"] < 0.5 and cases.track_for(c)[2, 6] == np.float32(c["bw_factor"] * cases.MALE_FS)


@pytest.mark.parametrize("float_class", [False, True], ids=CLASS_IDS)
def test_design_only_plans_report_the_vectors_rate_and_count(float_class):
    cls = cases.CLASSES[int(float_class)]
    manifest = cases.golden()["manifest"]
    for config, (voice, overrides) in cases.CONFIGS.items():
        plan = model5_plan(voice, overrides, cases.RATE, cases.CRATE, float_class=float_class, device=capi.DEVICE_NONE)
        m = manifest[cases.key(cases.cases_of(config)[0], config, cls)]
        assert abs(plan.info.internal_rate_hz - m["fs"]) < 2e-3, config
        counts = {manifest[cases.key(c, config, cls)]["n"] for c in cases.cases_of(config)}
        assert counts == {plan.output_count(cases.FRAMES)}, (config, counts)
        tr = cases.track_for(cases.cases_of(config)[0])
        for frames in (3, cases.FRAMES):
            out, _ = oracle.synthesize5(cases.oracle_config(config, cls[1]), tr[:frames], cases.CRATE)
            assert plan.output_count(frames) == out.size, (config, frames)
        plan.close()


@pytest.mark.parametrize("cls", cases.CLASSES, ids=CLASS_IDS)
def test_the_guarded_oracle_injects_nothing_outside_the_tube(cls):
    """Each constant-position product-rule track equals the same frames with fricVol 0 and fricPos 3.5, numerically (a +0
    may stand where the other has -0); the ramps, which pass through the tube first, do not."""
    consts = [c for c in cases.PRODUCT_CASES if c["form"] == "const"]
    ramps = [c for c in cases.PRODUCT_CASES if c["form"] == "ramp"]
    assert len(consts) == 7 and len(ramps) == 2
    todo = consts + ramps
    got = cases.synthesize_many([("male", cls[1], cases.track_for(c)) for c in todo])
    neutral = cases.synthesize_many([("male", cls[1], cases.track_for(c, neutral=True)) for c in todo])
    for c, a, b in zip(todo, got, neutral):
        assert a.size == b.size and np.isfinite(a).all() and np.isfinite(b).all(), c["name"]
        if c["form"] == "const":
            assert np.array_equal(a, b), c["name"]
        else:
            assert np.abs(a).max() > 0.0 and not np.array_equal(a, b), c["name"]
