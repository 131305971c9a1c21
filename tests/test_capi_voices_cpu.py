"""Plans of several voices (gvtm_plan_create_voices) on a design-only plan: creation, refusals, per-voice info and
output counts against the C oracle's vtmo_derive, and the single-voice entry points refused.  No GPU needed."""
import ctypes

import numpy as np
import pytest

import gama_tts_amd as g
from gama_tts_amd import capi

import oracle
from voice_cases import configs, create, oracle_config
from voice_files import VOICES, voice_path

TRACT_CM = [17.5, 15.0, 12.5, 10.0, 7.5]


def test_fixtures_differ_where_the_variants_do():
    tract = [float(g.read_config_file(voice_path(n))["vocal_tract_length"]) for n in VOICES]
    assert tract == TRACT_CM


def test_one_voice_plan_is_the_single_voice_plan():
    cfg = configs(names=["male"])
    vp = g.VoicesPlan(cfg, 250.0, capi.DEVICE_NONE)
    p = g.Plan(cfg[0], 250.0, capi.DEVICE_NONE)
    assert vp.n_voices == 1
    for field, _ in capi.Info._fields_:
        assert getattr(vp.info, field) == getattr(p.info, field), field
    for f in (0, 1, 2, 77, 500):
        assert vp.voice_output_count(0, f) == p.output_count(f)
        assert vp.voices_output_capacity(f) == p.output_capacity(f)
    for t in (capi.TABLE_FIR, capi.TABLE_SRC_H, capi.TABLE_SRC_DH, capi.TABLE_WAVETABLE):
        assert np.array_equal(vp.table(t), p.table(t))


@pytest.mark.parametrize("precision", [capi.PRECISION_F64, capi.PRECISION_MIXED, capi.PRECISION_F32])
@pytest.mark.parametrize("rate,delay,layout", [(44100.0, 1, 0), (44100.0, 2, 0), (22050.0, 1, 1), (48000.0, 3, 0)])
def test_five_voices_info_matches_the_oracle(precision, rate, delay, layout):
    cfgs = configs(rate, delay, precision, layout)
    vp = g.VoicesPlan(cfgs, 250.0, capi.DEVICE_NONE)
    assert vp.n_voices == 5
    seen_steps = set()
    for v, name in enumerate(VOICES):
        info = vp.voice_info(v)
        single = g.Plan(cfgs[v], 250.0, capi.DEVICE_NONE)
        ocfg = oracle_config(name, rate, delay, layout, precision)
        d = oracle.derive(ocfg)
        assert info.internal_sample_rate == d.sample_rate
        assert info.control_steps == d.control_steps
        assert info.upsampling == d.upsampling
        assert info.time_register_increment == d.time_register_increment
        assert info.phase_increment == d.phase_increment
        assert info.pad_size == d.pad_size
        assert info.fir_taps == d.fir_taps
        assert info.internal_sample_rate == single.info.internal_sample_rate
        assert info.output_rate == rate and info.section_delay == delay and info.precision == precision
        seen_steps.add(info.control_steps)
    # the variants' tract lengths give five different internal rates
    assert len(seen_steps) == 5
    # gvtm_plan_info reports voice 0
    v0 = vp.voice_info(0)
    for field, _ in capi.Info._fields_:
        assert getattr(vp.info, field) == getattr(v0, field), field


def test_male_up_samples_and_baby_down_samples_at_44k():
    vp = g.VoicesPlan(configs(), 250.0, capi.DEVICE_NONE)
    assert vp.voice_info(0).upsampling == 1 and vp.voice_info(0).internal_sample_rate < 44100
    assert vp.voice_info(4).upsampling == 0 and vp.voice_info(4).internal_sample_rate > 44100


@pytest.mark.parametrize("precision", [capi.PRECISION_F64, capi.PRECISION_F32])
def test_per_voice_counts_and_capacity(precision):
    cfgs = configs(precision=precision)
    vp = g.VoicesPlan(cfgs, 250.0, capi.DEVICE_NONE)
    singles = [g.Plan(c, 250.0, capi.DEVICE_NONE) for c in cfgs]
    for v, name in enumerate(VOICES):
        ocfg = oracle_config(name, 44100.0, 1, 0, precision)
        for f in (0, 1, 2, 3, 25, 250, 501):
            assert vp.voice_output_count(v, f) == singles[v].output_count(f) == oracle.output_count(ocfg, f)
    for f in (0, 1, 7, 250, 500, 2000):
        assert vp.voices_output_capacity(f) == max(p.output_capacity(f) for p in singles)
    lib = vp._lib
    assert lib.gvtm_voice_output_count(vp._h, 5, 10) == ctypes.c_size_t(-1).value
    assert lib.gvtm_voice_output_count(vp._h, -1, 10) == ctypes.c_size_t(-1).value


@pytest.mark.parametrize("field,value", [("output_rate", 48000.0), ("section_delay", 2),
                                         ("precision", capi.PRECISION_F32), ("tube_layout", capi.TUBE_30_18)])
def test_refuses_mismatched_model_keys(field, value):
    cfgs = configs()
    setattr(cfgs[3], field, value)
    rc, h = create(cfgs)
    assert rc == 1 and not h.value
    assert b"voice 3" in g.load_library().gvtm_last_error()


def test_refuses_no_voices_and_null_configs():
    lib = g.load_library()
    h = ctypes.c_void_p()
    assert lib.gvtm_plan_create_voices(None, 2, 250.0, capi.DEVICE_NONE, ctypes.byref(h)) == 1
    cfgs = configs()
    arr = (capi.Config * 5)(*cfgs)
    assert lib.gvtm_plan_create_voices(arr, 0, 250.0, capi.DEVICE_NONE, ctypes.byref(h)) == 1
    assert not h.value
    assert lib.gvtm_plan_create_voices(arr, 5, 250.0, capi.DEVICE_NONE, None) == 1


def test_refuses_a_bad_voice_config():
    cfgs = configs()
    cfgs[2].waveform = 7  # 0 pulse or 1 sine
    rc, h = create(cfgs)
    assert rc == 1 and not h.value
    assert b"voice 2" in g.load_library().gvtm_last_error()


def test_voice_info_out_of_range():
    vp = g.VoicesPlan(configs(), 250.0, capi.DEVICE_NONE)
    info = capi.Info()
    assert vp._lib.gvtm_plan_voice_info(vp._h, 5, ctypes.byref(info)) == 1
    assert vp._lib.gvtm_plan_voice_info(vp._h, -1, ctypes.byref(info)) == 1
    assert vp._lib.gvtm_plan_voice_count(None) < 0


def test_single_voice_entry_points_refused_on_a_multi_voice_plan():
    vp = g.VoicesPlan(configs(), 250.0, capi.DEVICE_NONE)
    lib = vp._lib
    params = np.zeros((2, 4, 16), dtype=np.float32)
    audio = np.zeros((2, 4096), dtype=np.float32)
    pcm = np.zeros((2, 4096), dtype=np.int16)
    p = params.ctypes.data
    assert lib.gvtm_synthesize_batch_device(vp._h, p, None, 2, 4, audio.ctypes.data, 4096, None, None, None) == 1
    assert b"voices" in lib.gvtm_last_error()
    assert lib.gvtm_synthesize_batch_host(vp._h, p, None, 2, 4, audio.ctypes.data, 4096, None, None) == 1
    assert lib.gvtm_synthesize_batch_host_pcm16(vp._h, p, None, 2, 4, pcm.ctypes.data, 4096, None, None, None) == 1
    s = ctypes.c_void_p()
    assert lib.gvtm_stream_create(vp._h, 2, ctypes.byref(s)) == 1 and not s.value
    tc = g.TrackConfig()
    tc.control_period_ms = 4
    assert lib.gvtm_synthesize_events_device(vp._h, ctypes.byref(tc), p, p, 2, 4, audio.ctypes.data, 4096,
                                             None, None, None, None, None) == 1
    assert b"voices" in lib.gvtm_last_error()
    # the voices entries on a design-only plan: no device
    ids = np.zeros(2, dtype=np.int32)
    assert lib.gvtm_synthesize_voices_host(vp._h, p, None, ids.ctypes.data, 4, 2, audio.ctypes.data, 4096, None, None) == 2


def test_single_voice_plan_takes_the_voices_entries_design_only():
    # a one-voice plan accepts both kinds of entry; design-only, both report the missing device
    vp = g.VoicesPlan(configs(names=["female"]), 250.0, capi.DEVICE_NONE)
    lib = vp._lib
    params = np.zeros((1, 4, 16), dtype=np.float32)
    audio = np.zeros((1, 4096), dtype=np.float32)
    ids = np.zeros(1, dtype=np.int32)
    assert lib.gvtm_synthesize_batch_host(vp._h, params.ctypes.data, None, 1, 4, audio.ctypes.data, 4096, None, None) == 2
    assert lib.gvtm_synthesize_voices_host(vp._h, params.ctypes.data, None, ids.ctypes.data, 4, 1, audio.ctypes.data, 4096, None, None) == 2


def test_model5_plans_have_one_voice():
    p = g.Plan(g.config5_from_dict(g.read_config_file(oracle.VOICE5_MALE)), 250.0, capi.DEVICE_NONE)
    assert p._lib.gvtm_plan_voice_count(p._h) == 1
    info = capi.Info()
    assert p._lib.gvtm_plan_voice_info(p._h, 0, ctypes.byref(info)) == 0 and info.model5 == 1
