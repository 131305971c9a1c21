"""Plans of several reference model 5 voices (gvtm_plan_create_model5_voices) on design-only plans: the five 5_male
variants (tests/golden/voice5_*.txt), per-voice info and output counts against the C oracle, the one-voice plan against
gvtm_plan_create_model5's, and the refusals.  No GPU needed."""
import ctypes

import numpy as np
import pytest

import gama_tts_amd as g
from gama_tts_amd import capi
import model5_cases as cases
import oracle
from voice_cases import configs5, create
from voice_files import VOICES, voice_path

VARIANT_KEYS = {"vocal_tract_length", "glottal_pulse_tn_min", "glottal_pulse_tn_max", "reference_glottal_pitch", "breathiness",
                "global_nasal_radius_coef", "global_radius_coef", "min_glottal_loss", "max_glottal_loss",
                "glottal_lowpass_cutoff", "intonation_factor", "mouth_impedance_radius"}


def test_fixtures_differ_exactly_where_the_variants_do():
    files = {n: g.read_config_file(voice_path(n, model5=True)) for n in VOICES}
    male = files["male"]
    assert male == g.read_config_file(oracle.VOICE5_MALE)
    for n in VOICES[1:]:
        assert set(files[n]) == set(male)
        differ = {k for k in male if files[n][k] != male[k]}
        assert differ and differ <= VARIANT_KEYS, (n, differ)
        assert float(files[n]["vocal_tract_length"]) == cases.TRACT_CM[n]
        assert files[n]["model"] == "5" and files[n]["output_rate"] == male["output_rate"]


def test_one_voice_plan_is_the_model5_plan():
    for name in ("male", "baby"):
        cfg = configs5(names=[name])
        vp = g.VoicesPlan(cfg, 250.0, capi.DEVICE_NONE)
        p = g.Plan(cfg[0], 250.0, capi.DEVICE_NONE)
        assert vp.n_voices == 1
        for field, _ in capi.Info._fields_:
            assert getattr(vp.info, field) == getattr(p.info, field), field
        assert vp.info.model5 == 1
        for f in (0, 1, 2, 77, 500):
            assert vp.voice_output_count(0, f) == p.output_count(f) == vp.output_count(f)
            assert vp.voices_output_capacity(f) == p.output_capacity(f)
        for t in (capi.TABLE_SRC_H, capi.TABLE_SRC_DH):
            assert np.array_equal(vp.table(t), p.table(t))


def test_five_voices_info_matches_the_oracle_and_the_issue_table():
    cfgs = configs5()
    vp = g.VoicesPlan(cfgs, 250.0, capi.DEVICE_NONE)
    assert vp.n_voices == 5
    for v, name in enumerate(VOICES):
        info = vp.voice_info(v)
        single = g.Plan(cfgs[v], 250.0, capi.DEVICE_NONE)
        for field, _ in capi.Info._fields_:
            assert getattr(info, field) == getattr(single.info, field), (name, field)
        _, rate = oracle.synthesize5(cases.voice_oracle_config(name), np.zeros((0, 16), np.float32))
        assert info.model5 == 1 and info.output_rate == cases.RATE
        assert abs(info.internal_rate_hz - rate) < 2e-3  # the oracle reports millihertz
        assert info.internal_rate_hz == pytest.approx((331.4 + 0.6 * 35.0) * 30 * 100 / cases.TRACT_CM[name], rel=1e-12)
        assert info.control_steps == round(rate / 250.0) == cases.STEPS_PER_FRAME[name]
        assert info.upsampling == 0  # every model 5 voice down-samples to 48 kHz
    for field, _ in capi.Info._fields_:
        assert getattr(vp.info, field) == getattr(vp.voice_info(0), field), field


def test_per_voice_counts_and_capacity():
    cfgs = configs5()
    vp = g.VoicesPlan(cfgs, 250.0, capi.DEVICE_NONE)
    singles = [g.Plan(c, 250.0, capi.DEVICE_NONE) for c in cfgs]
    for v, name in enumerate(VOICES):
        ocfg = cases.voice_oracle_config(name)
        frames = [0, 1, 2, 3, 25] + ([cases.OVERRUN_FRAMES[name]] if cases.OVERRUN_RATE.get(name) == cases.RATE else [])
        for f in frames:
            n = oracle.synthesize5(ocfg, np.zeros((f, 16), np.float32))[0].size
            assert vp.voice_output_count(v, f) == singles[v].output_count(f) == n, (name, f)
    for f in (0, 1, 7, 250, 500, 2000):
        cap = vp.voices_output_capacity(f)
        assert cap == max(p.output_capacity(f) for p in singles)
        # every utterance of at most f frames fits, those that run into the flush overrun included
        for v in range(5):
            assert all(vp.voice_output_count(v, k) <= cap for k in range(0, f + 1, max(1, f // 50)))
    lib = vp._lib
    for name in cases.NEW_VOICES:
        v, f = VOICES.index(name), cases.OVERRUN_FRAMES[name]
        at = vp if cases.OVERRUN_RATE[name] == cases.RATE else g.VoicesPlan(configs5(cases.OVERRUN_RATE[name]), 250.0, capi.DEVICE_NONE)
        info = at.voice_info(v)
        plain = -(-((f * info.control_steps + 2 * info.pad_size) << 16) // info.time_register_increment)
        assert at.voice_output_count(v, f) > plain  # the overrun's extra lap
        assert at.voices_output_capacity(f) >= at.voice_output_count(v, f)
    assert lib.gvtm_voice_output_count(vp._h, 5, 10) == ctypes.c_size_t(-1).value
    assert lib.gvtm_voice_output_count(vp._h, -1, 10) == ctypes.c_size_t(-1).value


def test_voices_may_differ_in_every_other_key():
    cfgs = configs5()
    cfgs[1].bypass = 1
    cfgs[2].constant_radius_mouth_impedance = 1
    cfgs[3].waveform = 1
    cfgs[4].noise_modulation = 0
    assert create(cfgs)[0] == 0


@pytest.mark.parametrize("field,value", [("output_rate", 44100.0), ("precision", capi.PRECISION_F32)])
def test_refuses_mismatched_model_keys(field, value):
    cfgs = configs5()
    setattr(cfgs[3], field, value)
    rc, h = create(cfgs)
    assert rc == 1 and not h.value
    assert b"voice 3" in g.load_library().gvtm_last_error()


def test_refuses_a_precision_other_than_f64():
    cfgs = configs5()
    for c in cfgs:
        c.precision = capi.PRECISION_MIXED
    rc, h = create(cfgs)
    assert rc == 1 and not h.value
    assert b"fp64" in g.load_library().gvtm_last_error()


def test_refuses_no_voices_and_null_configs():
    lib = g.load_library()
    h = ctypes.c_void_p()
    assert lib.gvtm_plan_create_model5_voices(None, 2, 250.0, capi.DEVICE_NONE, ctypes.byref(h)) == 1
    arr = (capi.Config5 * 5)(*configs5())
    assert lib.gvtm_plan_create_model5_voices(arr, 0, 250.0, capi.DEVICE_NONE, ctypes.byref(h)) == 1
    assert not h.value
    assert lib.gvtm_plan_create_model5_voices(arr, 5, 250.0, capi.DEVICE_NONE, None) == 1


def test_refuses_a_bad_voice_and_names_it():
    cfgs = configs5()
    cfgs[2].vocal_tract_length = 25.0  # 352.4 * 30 * 100 / 25 = 42.3 kHz: below the 50 kHz model 5 needs
    rc, h = create(cfgs)
    assert rc == 1 and not h.value
    msg = g.load_library().gvtm_last_error()
    assert msg.startswith(b"voice 2: ") and b"50 kHz" in msg
    cfgs = configs5()
    cfgs[0].vocal_tract_length = 25.0
    assert create(cfgs)[0] == 1 and g.load_library().gvtm_last_error().startswith(b"voice 0: ")
    # a one-voice plan reports as gvtm_plan_create_model5 does
    assert create(cfgs[:1])[0] == 1 and not g.load_library().gvtm_last_error().startswith(b"voice")


def test_voice_info_out_of_range():
    vp = g.VoicesPlan(configs5(), 250.0, capi.DEVICE_NONE)
    info = capi.Info()
    assert vp._lib.gvtm_plan_voice_info(vp._h, 5, ctypes.byref(info)) == 1
    assert vp._lib.gvtm_plan_voice_info(vp._h, -1, ctypes.byref(info)) == 1


def test_mixing_model5_and_other_configs_is_a_type_error():
    with pytest.raises(TypeError):
        g.VoicesPlan([configs5(names=["male"])[0], g.config_from_dict(g.read_config_file(oracle.VOICE_MALE), 48000.0)],
                     250.0, capi.DEVICE_NONE)


def test_single_voice_entry_points_refused_on_a_five_voice_plan():
    vp = g.VoicesPlan(configs5(), 250.0, capi.DEVICE_NONE)
    lib = vp._lib
    params = np.zeros((2, 4, 16), dtype=np.float32)
    audio = np.zeros((2, 8192), dtype=np.float32)
    pcm = np.zeros((2, 8192), dtype=np.int16)
    p = params.ctypes.data
    assert lib.gvtm_synthesize_batch_device(vp._h, p, None, 2, 4, audio.ctypes.data, 8192, None, None, None) == 1
    assert b"5 voices" in lib.gvtm_last_error()
    assert lib.gvtm_synthesize_batch_host(vp._h, p, None, 2, 4, audio.ctypes.data, 8192, None, None) == 1
    assert lib.gvtm_synthesize_batch_host_pcm16(vp._h, p, None, 2, 4, pcm.ctypes.data, 8192, None, None, None) == 1
    s = ctypes.c_void_p()
    assert lib.gvtm_stream_create(vp._h, 2, ctypes.byref(s)) == 1 and not s.value
    assert b"gvtm_stream_create" in lib.gvtm_last_error()
    tc = g.TrackConfig()
    tc.control_period_ms = 4
    assert lib.gvtm_synthesize_events_device(vp._h, ctypes.byref(tc), p, p, 2, 4, audio.ctypes.data, 8192,
                                             None, None, None, None, None) == 1
    assert b"gvtm_synthesize_events_device" in lib.gvtm_last_error()
    # the voices entries on a design-only plan: no device (not a refusal)
    ids = np.zeros(2, dtype=np.int32)
    assert lib.gvtm_synthesize_voices_host(vp._h, p, None, ids.ctypes.data, 4, 2, audio.ctypes.data, 8192, None, None) == 2


def test_one_voice_model5_plan_takes_the_voices_entries_design_only():
    # before plans of several model 5 voices, the voices entries refused model 5 plans (GVTM_ERR_INVALID_ARGUMENT)
    p = g.Plan(configs5(names=["female"])[0], 250.0, capi.DEVICE_NONE)
    lib = p._lib
    params = np.zeros((1, 4, 16), dtype=np.float32)
    audio = np.zeros((1, 8192), dtype=np.float32)
    ids = np.zeros(1, dtype=np.int32)
    assert lib.gvtm_synthesize_voices_host(p._h, params.ctypes.data, None, ids.ctypes.data, 4, 1, audio.ctypes.data, 8192, None, None) == 2
    assert lib.gvtm_synthesize_voices_device(p._h, params.ctypes.data, None, ids.ctypes.data, 4, 1, audio.ctypes.data, 8192,
                                             None, None, None) == 2
