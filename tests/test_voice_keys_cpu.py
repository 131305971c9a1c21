"""The voice-configuration keys of tests/voice_key_cases.py without a GPU: the oracle on every set against vectors of the
real reference (tests/golden/voice_keys_golden.npz), the host designs (double and float) against the oracle's for every
set x cell and for the model 5 sets in both classes, and the table itself: it moves every key that nothing else moves,
its plans of several voices separate every such key, and the GPU tests' track hears every such key."""
import ctypes
import functools
import hashlib
import json
import os

import numpy as np
import pytest

from gama_tts_amd import capi
import golden_cases
import model5_cases
import oracle
import voice_files
import voice_key_cases as cases
from parity_rules import TOL, TOL5, within
from voice_cases import male_plan, model5_plan

HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(os.path.join(HERE, "golden", "voice_keys_golden.npz"), allow_pickle=False)
    data = {k: z[k] for k in z.files}
    data["manifest"] = json.loads(bytes(data.pop("manifest_json")).decode())
    return data


def oracle_config(cell, overrides):
    return oracle.male_config(cell.rate, cell.delay, cell.layout, cell.float_model, **overrides)


def oracle5_config(overrides, float_model):
    return model5_cases.voice_oracle_config("male", cases.RATE5, float_model, overrides)


# ---- the oracle against the reference -----------------------------------------------------------------------------------------

def check_vector(out, key):
    data = fixture()
    m = data["manifest"][key]
    assert out.size == m["n"], key
    assert np.array_equal(out[:: golden_cases.DIGEST_STRIDE], data[key + "__strided"]), key
    assert hashlib.sha256(out.tobytes()).hexdigest() == m["sha256"], key
    return m


def test_fixture_holds_every_run_of_the_table_and_nothing_else():
    assert sorted(fixture()["manifest"]) == sorted(r[0] for r in cases.reference_runs())
    assert len(fixture()["manifest"]) == len(cases.SETS) * 6 + len(cases.SETS5) * 2


@pytest.mark.parametrize("cell", cases.CELLS, ids=cases.CELL_IDS)
@pytest.mark.parametrize("name", list(cases.SETS))
def test_oracle_matches_the_reference(name, cell):
    cfg = oracle_config(cell, cases.SETS[name])
    m = check_vector(oracle.synthesize(cfg, cases.track()), cases.fixture_key(name, cell.model))
    od = oracle.derive(cfg)
    assert m["rate"] == cell.rate and od.control_steps * cases.FRAMES == m["steps"] and od.sample_rate == int(m["fs"])
    assert od.control_steps == cases.STEPS.get(name, cases.MALE_STEPS)[cases.steps_index(cell)]


@pytest.mark.parametrize("model,float_model", cases.MODELS5)
@pytest.mark.parametrize("name", list(cases.SETS5))
def test_oracle5_matches_the_reference(name, model, float_model):
    out, rate = oracle.synthesize5(oracle5_config(cases.SETS5[name], float_model), cases.track())
    m = check_vector(out, cases.fixture_key(name, model))
    assert abs(rate - m["fs"]) < 2e-3


# ---- the host design against the oracle's -------------------------------------------------------------------------------------

@pytest.mark.parametrize("cell", cases.CELLS, ids=cases.CELL_IDS)
@pytest.mark.parametrize("name", list(cases.SETS))
def test_design_matches_oracle_bit_for_bit(name, cell):
    """What test_capi_cpu.py's test_design_matches_oracle_bit_for_bit and its float twin assert, at this set."""
    plan = male_plan(cases.SETS[name], cell.rate, cell.delay, precision=cell.precision, layout=cell.layout, device=capi.DEVICE_NONE)
    ocfg = oracle_config(cell, cases.SETS[name])
    od = oracle.derive(ocfg)
    i = plan.info
    assert i.precision == cell.precision
    assert (i.internal_sample_rate, i.control_steps, i.fir_taps) == (od.sample_rate, od.control_steps, od.fir_taps)
    assert (i.time_register_increment, i.phase_increment, i.pad_size, i.upsampling) == \
        (od.time_register_increment, od.phase_increment, od.pad_size, od.upsampling)
    L = oracle.lib()
    if cell.float_model:
        fir, h, dh, wt = (np.empty(n, dtype=np.float32) for n in (401, 3328, 3328, 512))
        n = L.vtmo_fir_coefficients_f32(fir.ctypes.data)
        L.vtmo_src_filter_f32(h.ctypes.data, dh.ctypes.data)
        L.vtmo_wavetable_f32(ctypes.byref(ocfg), od.sample_rate, wt.ctypes.data)
    else:
        fir, h, dh, wt = (np.empty(n) for n in (401, 3328, 3328, 512))
        n = L.vtmo_fir_coefficients(fir.ctypes.data)
        L.vtmo_src_filter(h.ctypes.data, dh.ctypes.data)
        L.vtmo_wavetable(ctypes.byref(ocfg), od.sample_rate, wt.ctypes.data)
    assert np.array_equal(plan.table(capi.TABLE_FIR), fir[:n].astype(np.float64))
    assert np.array_equal(plan.table(capi.TABLE_SRC_H), h.astype(np.float64))
    assert np.array_equal(plan.table(capi.TABLE_SRC_DH), dh.astype(np.float64))
    assert np.array_equal(plan.table(capi.TABLE_WAVETABLE), wt.astype(np.float64))
    for frames in cases.COUNT_FRAMES:
        assert plan.output_count(frames) == oracle.output_count(ocfg, frames), frames
    assert plan.output_count(cases.FRAMES) == fixture()["manifest"][cases.fixture_key(name, cell.model)]["n"]


def test_pulse_set_sits_on_the_tie_of_the_wavetable_division():
    """512 * tp / 100 is 179.5 exactly; which side rint() takes follows from the rounding of tp / 100 in the design's type,
    so the set's wavetable is not the male voice's in either, whatever the side."""
    tp = cases.SETS["pulse"]["glottal_pulse_tp"]
    assert 512.0 * tp / 100.0 == 179.5
    for cell in cases.CELLS[:3]:
        got = male_plan(cases.SETS["pulse"], cell.rate, cell.delay, precision=cell.precision, device=capi.DEVICE_NONE).table(capi.TABLE_WAVETABLE)
        male = male_plan(None, cell.rate, cell.delay, precision=cell.precision, device=capi.DEVICE_NONE).table(capi.TABLE_WAVETABLE)
        assert not np.array_equal(got, male), cell.name
        assert oracle.derive(oracle_config(cell, cases.SETS["pulse"])).table_div1 in (179, 180)


@pytest.mark.parametrize("model,float_model", cases.MODELS5)
@pytest.mark.parametrize("name", list(cases.SETS5))
def test_model5_design_matches_the_reference_and_the_oracle(name, model, float_model):
    """What test_capi_model5_cpu.py and test_capi_model5_float_cpu.py assert of the male voice, at this set."""
    m = fixture()["manifest"][cases.fixture_key(name, model)]
    plan = model5_plan("male", cases.SETS5[name], cases.RATE5, cases.CRATE, float_class=bool(float_model), device=capi.DEVICE_NONE)
    ocfg = oracle5_config(cases.SETS5[name], float_model)
    i = plan.info
    assert i.model5 == 1 and i.precision == (capi.PRECISION_F32 if float_model else capi.PRECISION_F64)
    if float_model:
        _, oracle_rate = oracle.synthesize5(ocfg, np.zeros((0, 16), np.float32))
        assert int(np.float32(i.internal_rate_hz) * np.float32(1000.0)) == round(oracle_rate * 1000.0)
        assert abs(i.internal_rate_hz - m["fs"]) < 2e-3 and i.internal_rate_hz == float(np.float32(i.internal_rate_hz))
    else:
        assert abs(i.internal_rate_hz - m["fs"]) < 1e-9 and i.internal_sample_rate == int(m["fs"])
    assert i.control_steps * cases.FRAMES == m["steps"]
    assert plan.output_count(cases.FRAMES) == m["n"]
    assert i.output_rate == cases.RATE5 and i.upsampling == int(cases.RATE5 >= m["fs"])
    for frames in cases.COUNT_FRAMES:
        assert plan.output_count(frames) == oracle.synthesize5(ocfg, np.zeros((frames, 16), np.float32))[0].size, frames
    if name == "m5_acoustics":  # the temperature moves the internal rate and the steps per frame
        assert i.control_steps != model5_cases.STEPS_PER_FRAME["male"]


# ---- completeness -------------------------------------------------------------------------------------------------------------

def moved_elsewhere(case_lists, files, keep=()):
    """The keys that the overrides of other fixture lists move, or in which the voice files differ."""
    moved = {k for cs in case_lists for c in cs for k in c["overrides"]}
    voices = [oracle.read_config_file(p) for p in files]
    moved |= {k for k in voices[0] if any(v.get(k) != voices[0][k] for v in voices[1:])}
    return moved - set(keep)


def test_key_lists_are_the_fields_that_nothing_else_moves():
    skip = set(cases.STRUCTURAL) | set(cases.FLAGS)
    elsewhere = moved_elsewhere([golden_cases.CASES], [voice_files.voice_path(v) for v in voice_files.VOICES])
    assert set(cases.field_keys(capi.Config)) - skip - elsewhere == set(cases.KEYS)
    # model 5: loss_factor and the two glottal losses move once, all together (radius_coefs_m5), and stay on the list; so
    # does glottal_lowpass_cutoff, which takes two values in the voice files
    elsewhere5 = moved_elsewhere(model5_cases.CASES.values(), [voice_files.voice_path(v, True) for v in voice_files.VOICES],
                                 keep=("loss_factor", "min_glottal_loss", "max_glottal_loss", "glottal_lowpass_cutoff"))
    assert set(cases.field_keys(capi.Config5)) - skip - elsewhere5 == set(cases.KEYS5)


@pytest.mark.parametrize("keys,sets,path", [(cases.KEYS, cases.SETS, oracle.VOICE_MALE), (cases.KEYS5, cases.SETS5, oracle.VOICE5_MALE)],
                         ids=["models0to4", "model5"])
def test_every_key_moves_in_a_set(keys, sets, path):
    male = oracle.read_config_file(path)
    for key in keys:
        movers = [name for name, ov in sets.items() if key in ov and float(ov[key]) != float(male[key])]
        assert movers, key
        assert cases.owner(key, sets) == movers[0]
    for name, ov in sets.items():  # and no set names a key the voice file does not have
        assert set(ov) <= set(male), name


def test_every_key_separates_two_voices_of_the_plans_of_several_voices():
    lists = cases.voice_lists()
    assert [len(v) for v in lists.values()] == [8, 8]
    assert lists["male_first"][0] == {} and lists["male_last"][-1] == {}
    assert sorted(map(repr, lists["male_first"])) == sorted(map(repr, lists["male_last"]))
    for key in cases.KEYS:
        assert cases.separating_pair(key) is not None, key
    for key in cases.KEYS5:
        assert cases.separating_pair(key, cases.VOICE_NAMES5) is not None, key
    # temperature and length give the eight voices three internal rates
    cell = cases.CELLS[0]
    steps = {oracle.derive(oracle_config(cell, ov)).control_steps for ov in lists["male_first"]}
    assert steps == {79, 80, 87}


# ---- sensitivity --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cell", [cases.CELLS[0], cases.CELLS[2]], ids=["double", "float"])
def test_track_hears_every_key(cell):
    """A key whose move the track cannot hear proves nothing on the device: the key alone at its set's value changes the
    oracle's output -- its length, or some sample by more than the loosest bar of the GPU tests (mixed: 1e-5 of peak), so
    that a kernel on the male voice's constant fails in every precision."""
    tr = cases.track()
    male = oracle.synthesize(oracle_config(cell, {}), tr)
    for key in cases.KEYS:
        out = oracle.synthesize(oracle_config(cell, {key: cases.SETS[cases.owner(key)][key]}), tr)
        assert out.size != male.size or not within(out, male, max(TOL.values())), key


@pytest.mark.parametrize("model,float_model", cases.MODELS5)
def test_track_hears_every_model5_key(model, float_model):
    tr = cases.track()
    male, _ = oracle.synthesize5(oracle5_config({}, float_model), tr)
    for key in cases.KEYS5:
        out, _ = oracle.synthesize5(oracle5_config({key: cases.SETS5[cases.owner(key, cases.SETS5)][key]}, float_model), tr)
        assert out.size != male.size or np.abs(out.astype(np.float64) - male).max() > TOL5 * np.abs(male).max(), key


def test_batches_of_the_gpu_tests():
    params, frames = cases.batch()
    assert params.shape == (6, cases.FRAMES, 16) and sorted(set(frames)) == list(cases.CUTS)
    assert 0 in frames[:4] and len(set(frames[:4])) == 4  # a four-row workgroup: rows of different length, one empty
    assert sum(cases.STREAM_PIECES) == cases.FRAMES
    for n in (len(cases.VOICE_NAMES), len(cases.VOICE_NAMES5)):
        p, ids, fr = cases.voices_batch(n)
        assert ids.size == 3 * n <= 40 and (np.bincount(ids) == 3).all()
        for b in range(ids.size):
            assert np.array_equal(p[b, : fr[b]], cases.track()[: fr[b]]) and not p[b, fr[b]:].any()
        assert all(sorted(fr[ids == v])[1:] == [13, cases.FRAMES] for v in range(n))
