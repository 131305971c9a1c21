"""Plans of several voices of the float class of reference model 5 (gvtm_plan_create_model5_float_voices) on design-only
plans and the diagnostics library: every voice designed as its single-voice float plan (gvtm_plan_create_model5_float) is,
the refusals, the entries a design-only plan answers, and the kernel shape a launch of several voices takes (the rule of
the single-voice float class: chunk 60, 84 992 B, up to 256 utterances; chunk 56, 80 800 B, beyond).  No GPU needed."""
import ctypes

import numpy as np
import pytest

import gama_tts_amd as g
from gama_tts_amd import capi
import model5_cases as cases
from voice_cases import configs5, track_configs
from voice_files import VOICES
from voices5_float_cases import configs5f, create, float_voices_plan, single_float_plan

NONE = capi.DEVICE_NONE
LDS_CHUNK60, LDS_CHUNK56 = 84992, 80800


def test_the_library_exports_the_entry_and_no_debug_hook():
    lib = g.load_library()
    assert hasattr(lib, "gvtm_plan_create_model5_float_voices")
    assert not hasattr(lib, "gvtm_debug_launch_shape")


def test_every_voice_is_designed_as_its_single_voice_float_plan():
    cfgs = configs5f()
    vp = float_voices_plan(cfgs, device=NONE)
    assert vp.n_voices == 5 == vp._lib.gvtm_plan_voice_count(vp._h)
    for v, name in enumerate(VOICES):
        info, single = vp.voice_info(v), single_float_plan(cfgs[v], device=NONE)
        for field, _ in capi.Info._fields_:
            assert getattr(info, field) == getattr(single.info, field), (name, field)
        assert info.model5 == 1 and info.precision == capi.PRECISION_F32 and info.output_rate == cases.RATE
        assert info.internal_rate_hz == single.info.internal_rate_hz == float(np.float32(info.internal_rate_hz))
        assert info.control_steps == cases.STEPS_PER_FRAME[name]
    assert [vp.voice_info(v).control_steps for v in range(5)] == [242, 282, 338, 423, 564]
    for field, _ in capi.Info._fields_:
        assert getattr(vp.info, field) == getattr(vp.voice_info(0), field), field


def test_per_voice_counts_at_the_overrun_lengths_and_the_capacity():
    for rate in sorted(set(cases.OVERRUN_RATE.values())):
        cfgs = configs5f(rate)
        vp = float_voices_plan(cfgs, device=NONE)
        singles = [single_float_plan(c, device=NONE) for c in cfgs]
        for v, name in enumerate(VOICES):
            frames = [0, 1, 2, 3, 25, 500]
            if cases.OVERRUN_RATE.get(name) == rate:
                f = cases.OVERRUN_FRAMES[name]
                frames += [f, f + 1]
                assert vp.voice_output_count(v, f) > vp.voice_output_count(v, f + 1)  # the overrun's extra lap
            for f in frames:
                assert vp.voice_output_count(v, f) == singles[v].output_count(f), (name, f)
        for f in (0, 1, 7, 250, 500, 2000):
            assert vp.voices_output_capacity(f) == max(p.output_capacity(f) for p in singles)
    lib = vp._lib
    assert lib.gvtm_voice_output_count(vp._h, 5, 10) == ctypes.c_size_t(-1).value
    assert lib.gvtm_voice_output_count(vp._h, -1, 10) == ctypes.c_size_t(-1).value


def test_one_voice_plan_is_the_float_plan():
    cfg = configs5f(names=["baby"])
    vp, p = float_voices_plan(cfg, device=NONE), single_float_plan(cfg[0], device=NONE)
    assert vp.n_voices == 1
    for field, _ in capi.Info._fields_:
        assert getattr(vp.info, field) == getattr(p.info, field), field
    for f in (0, 1, 77, cases.OVERRUN_FRAMES["baby"]):
        assert vp.voice_output_count(0, f) == p.output_count(f) == vp.output_count(f)
        assert vp.voices_output_capacity(f) == p.output_capacity(f)
    for t in (capi.TABLE_SRC_H, capi.TABLE_SRC_DH):
        assert np.array_equal(vp.table(t), p.table(t))


def test_the_converter_tables_depend_on_no_voice():
    """One set of float converter tables on the device serves every voice: every voice's design has the same."""
    ref = None
    for cfg in configs5f() + configs5f(44100.0, overrides={0: dict(bypass=1, waveform=1)}):
        p = single_float_plan(cfg, device=NONE)
        tables = [p.table(t) for t in (capi.TABLE_SRC_H, capi.TABLE_SRC_DH)]
        ref = ref or tables
        assert all(np.array_equal(a, b) for a, b in zip(tables, ref))


@pytest.mark.parametrize("field,value", [("output_rate", 44100.0), ("precision", capi.PRECISION_F64)])
def test_refuses_mismatched_model_keys(field, value):
    cfgs = configs5f()
    setattr(cfgs[3], field, value)
    rc, h, msg = create(cfgs)
    assert rc == 1 and not h.value and b"voice 3" in msg


def test_refuses_the_double_class_and_the_double_entry_still_refuses_the_float_class():
    rc, h, msg = create(configs5())  # every voice GVTM_PRECISION_F64
    assert rc == 1 and not h.value and b"fp32" in msg
    rc, h, msg = create(configs5f(), entry="gvtm_plan_create_model5_voices")
    assert rc == 1 and not h.value and b"fp64" in msg


def test_refuses_a_voice_the_float_design_refuses_and_names_it():
    cfgs = configs5f()
    cfgs[2].vocal_tract_length = 25.0  # 352.4 * 30 * 100 / 25 = 42.3 kHz: below the 50 kHz model 5 needs
    rc, h, msg = create(cfgs)
    assert rc == 1 and not h.value and msg.startswith(b"voice 2: ") and b"50 kHz" in msg
    cfgs = configs5f()
    cfgs[0].vocal_tract_length = 25.0
    rc, h, msg = create(cfgs)
    assert rc == 1 and msg.startswith(b"voice 0: ")


def test_refuses_no_voices_and_null_pointers():
    cfgs = configs5f()
    assert create(cfgs, n=0)[0] == 1
    rc, h, _ = create(None, n=2)
    assert rc == 1 and not h.value
    assert create(cfgs, plan_out=False)[0] == 1


def test_voices_may_differ_in_every_other_key():
    cfgs = configs5f()
    cfgs[1].bypass = 1
    cfgs[2].constant_radius_mouth_impedance = 1
    cfgs[3].waveform = 1
    cfgs[4].noise_modulation = 0
    assert create(cfgs)[0] == 0


def test_a_design_only_plan_has_no_device_and_takes_voice_tracks():
    vp = float_voices_plan(device=NONE)
    lib = vp._lib
    params = np.zeros((2, 4, 16), dtype=np.float32)
    audio = np.zeros((2, 8192), dtype=np.float32)
    ids = np.zeros(2, dtype=np.int32)
    p = params.ctypes.data
    assert lib.gvtm_synthesize_voices_host(vp._h, p, None, ids.ctypes.data, 4, 2, audio.ctypes.data, 8192, None, None) == 2
    assert lib.gvtm_synthesize_voices_device(vp._h, p, None, ids.ctypes.data, 4, 2, audio.ctypes.data, 8192, None, None, None) == 2
    s = ctypes.c_void_p()
    assert lib.gvtm_stream_create_voices(vp._h, ids.ctypes.data, 2, ctypes.byref(s)) == 2 and not s.value
    vp.set_voice_tracks(track_configs(model5=True))
    with pytest.raises(capi.GvtmError):
        vp.set_voice_tracks(track_configs(model5=True)[:4])
    # five voices: the single-voice entries would not know which one to synthesize
    assert lib.gvtm_synthesize_batch_host(vp._h, p, None, 2, 4, audio.ctypes.data, 8192, None, None) == 1
    assert b"5 voices" in lib.gvtm_last_error()
    assert lib.gvtm_stream_create(vp._h, 2, ctypes.byref(s)) == 1 and not s.value
    # a one-voice plan takes them (no device here, so GVTM_ERR_NO_DEVICE rather than a refusal)
    one = float_voices_plan(configs5f(names=["female"]), device=NONE)
    assert lib.gvtm_synthesize_batch_host(one._h, p, None, 2, 4, audio.ctypes.data, 8192, None, None) == 2
    assert lib.gvtm_synthesize_voices_host(one._h, p, None, ids.ctypes.data, 4, 2, audio.ctypes.data, 8192, None, None) == 2


def test_the_shape_of_a_voices_launch_follows_the_float_class_rule():
    lib = g.load_library(diagnostics=True)

    def shape(plan, batch):
        out = (ctypes.c_size_t * 3)()
        assert lib.gvtm_debug_launch_shape(plan._h, batch, 1, out) == 0
        assert out[0] == 1 and out[1] == 0  # one utterance per workgroup; the ring is a constant of the kernel
        return out[2]

    plan = g.VoicesPlan(configs5f(), 250.0, NONE, diagnostics=True, float_model5=True)
    assert [shape(plan, b) for b in (1, 45, 256)] == [LDS_CHUNK60] * 3
    assert [shape(plan, b) for b in (257, 512, 4096)] == [LDS_CHUNK56] * 3
    for rows, lds in ((1, LDS_CHUNK60), (2, LDS_CHUNK56)):
        forced = float_voices_plan(device=NONE, rows=rows)
        assert [shape(forced, b) for b in (1, 256, 257, 4096)] == [lds] * 4
