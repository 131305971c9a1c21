"""Host side of the float class of reference model 5 (gvtm_plan_create_model5_float: VocalTractModel5<float,1>) on all five
5_male variants (tests/golden/voice5_*.txt), without a GPU: design-only plans against the float oracle and the reference's
vectors (tests/golden/voices5f_golden.npz) -- internal rate, driver loop, output counts through every voice's flush overrun
-- and the ends of the range of output rates the class accepts: a down-sampling pad of 96 at the low end, 3 x the internal
rate at the high end.  The ends are found here, per voice, from the converter's own float arithmetic
(SampleRateConverter<float>::initializeConversion as oracle/vtm_oracle_body.inc:317-325 restates it), not taken from the
product."""
import ctypes
import functools

import numpy as np
import pytest

import gama_tts_amd as g
from gama_tts_amd import capi
import model5_cases as cases
import oracle
from voice_cases import model5_plan
from voice_files import VOICES, voice_path

f32 = np.float32
# (voice, output rate, control rate, steps per frame)
CONTROL_RATE_CASES = [("male", 16000.0, 1000.0, 60), ("female", 16000.0, 1000.0, 70), ("small_child", 22050.0, 500.0, 211),
                      ("baby", 32000.0, 200.0, 705)]


_plan = functools.partial(model5_plan, float_class=True, device=capi.DEVICE_NONE)  # design-only, the float class


def _oracle_count(voice, rate, frames, crate=cases.CRATE):
    return oracle.synthesize5(cases.voice_oracle_config(voice, rate, 1), np.zeros((frames, 16), np.float32), crate)[0].size


def internal_rate(voice):
    """VocalTractModel5<float,1>'s internal rate (VocalTractModel5.h:462-465), every operation in float."""
    d = oracle.read_config_file(voice_path(voice, True))
    length = f32(d["vocal_tract_length_offset"]) + f32(d["vocal_tract_length"])
    speed = f32(331.4) + f32(0.6) * f32(d["temperature"])
    return (speed * f32(30) * f32(100)) / length


def converter(fs, rate):
    """-> (ratio, time register increment, pad) of SampleRateConverter<float> for an output rate."""
    ratio = f32(rate) / fs
    assert ratio.dtype == np.float32
    time_inc = int(np.rint(65536.0 / float(ratio)))  # (formed in double: SampleRateConverter.h:145)
    rounded_ratio = f32(65536.0 / time_inc)
    pad = 13 if ratio >= f32(1.0) else int(f32(13.0) / rounded_ratio) + 1
    return ratio, time_inc, pad


def _first_float(lo, hi, pred):
    """The smallest float32 in (lo, hi] for which pred holds (pred(lo) false, pred(hi) true, monotone in between): a
    bisection over the bit patterns, which order positive floats as their values do."""
    a, b = int(f32(lo).view(np.uint32)), int(f32(hi).view(np.uint32))
    assert not pred(f32(lo)) and pred(f32(hi))
    while b - a > 1:
        mid = (a + b) // 2
        if pred(np.uint32(mid).view(np.float32)):
            b = mid
        else:
            a = mid
    return np.uint32(a).view(np.float32), np.uint32(b).view(np.float32)


def _refused(voice, rate):
    with pytest.raises(g.GvtmError) as ei:
        _plan(voice, rate=float(rate))
    return ei.value.status


@pytest.mark.parametrize("voice", VOICES)
def test_rate_steps_and_branch(voice):
    fs = internal_rate(voice)
    for rate in (cases.RATE, 22050.0, 176400.0):
        i = _plan(voice, rate=rate).info
        assert i.model5 == 1 and i.precision == capi.PRECISION_F32 and i.output_rate == rate
        assert i.internal_rate_hz == float(fs)  # (a float, and the class's)
        assert i.control_steps == cases.STEPS_PER_FRAME[voice] == round(float(fs) / cases.CRATE)
        ratio, time_inc, pad = converter(fs, rate)
        assert i.upsampling == int(rate >= float(fs)) == int(ratio >= 1.0)
        assert i.time_register_increment == time_inc and i.pad_size == pad
    # what the reference's class reports for the voice
    m = cases.load("voices5f")["manifest"]
    for c in cases.FLOAT_CASES:
        if c["voice"] == voice:
            assert abs(float(fs) - m[c["name"]]["fs"]) < 2e-3
            assert m[c["name"]]["steps"] == cases.STEPS_PER_FRAME[voice] * m[c["name"]]["frames"]


@pytest.mark.parametrize("case", cases.FLOAT_CASES, ids=lambda c: c["name"])
def test_output_count_of_the_reference_vectors(case):
    m = cases.load("voices5f")["manifest"][case["name"]]
    plan = _plan(case["voice"], case["overrides"], case["rate"], case["crate"])
    assert plan.output_count(m["frames"]) == m["n"] <= plan.output_capacity(m["frames"])


@pytest.mark.parametrize("voice", VOICES)
def test_output_counts_follow_the_float_oracle(voice):
    """Every length up to 40 frames at 48 kHz, and the three lengths around the voice's flush overrun (male: 106 frames at
    44.1 kHz, tests/model5_cases.py)."""
    plan = _plan(voice)
    counts = {f: plan.output_count(f) for f in range(41)}
    for f, n in counts.items():
        assert n == _oracle_count(voice, cases.RATE, f), f
    assert plan.output_capacity(40) >= max(counts.values())
    ovr, rate = (106, 44100.0) if voice == "male" else (cases.OVERRUN_FRAMES[voice], cases.OVERRUN_RATE[voice])
    plan = _plan(voice, rate=rate)
    n = {f: plan.output_count(f) for f in (ovr - 1, ovr, ovr + 1)}
    for f in n:
        assert n[f] == _oracle_count(voice, rate, f), f
    assert n[ovr] > n[ovr + 1] > n[ovr - 1]
    assert plan.output_capacity(ovr + 1) >= n[ovr] and plan.output_capacity(ovr) >= n[ovr]


@pytest.mark.parametrize("voice", VOICES)
def test_lowest_accepted_rate_has_pad_96(voice):
    fs = internal_rate(voice)
    below, lowest = _first_float(1000.0, 0.5 * float(fs), lambda r: converter(fs, r)[2] <= cases.MAX_PAD)
    assert converter(fs, lowest)[2] == cases.MAX_PAD and converter(fs, below)[2] == cases.MAX_PAD + 1
    plan = _plan(voice, rate=float(lowest))
    assert plan.info.pad_size == cases.MAX_PAD and plan.info.upsampling == 0
    assert plan.info.time_register_increment == converter(fs, lowest)[1]
    for f in range(4):
        assert plan.output_count(f) == _oracle_count(voice, float(lowest), f) <= plan.output_capacity(f)
    assert _refused(voice, below) == 1
    assert b"down-sampling range" in g.load_library().gvtm_last_error()


def test_the_pad_96_vectors_have_pad_96():
    for voice, rate, what in cases.LIMITS:
        fs = internal_rate(voice)
        if what == "pad96":
            assert converter(fs, rate)[2] == cases.MAX_PAD == _plan(voice, rate=rate).info.pad_size
        else:
            assert converter(fs, rate)[0] == f32(3.0)


@pytest.mark.parametrize("voice", VOICES)
def test_highest_accepted_rate_is_three_times_the_internal_rate(voice):
    fs = internal_rate(voice)
    highest, above = _first_float(2.0 * float(fs), 4.0 * float(fs), lambda r: converter(fs, r)[0] > f32(3.0))
    assert converter(fs, highest)[0] <= f32(3.0) < converter(fs, above)[0]
    if voice != "male":  # (male's 60 411.43 Hz has no float that is 3.0 times it: its highest ratio is 2.9999998)
        assert float(fs) * 3.0 == float(f32(3.0) * fs) <= float(highest) and converter(fs, highest)[0] == f32(3.0)
    plan = _plan(voice, rate=float(highest))
    assert plan.info.upsampling == 1 and plan.info.pad_size == 13
    assert plan.info.time_register_increment == converter(fs, highest)[1]
    for f in range(4):
        assert plan.output_count(f) == _oracle_count(voice, float(highest), f) <= plan.output_capacity(f)
    assert _refused(voice, above) == 1
    assert b"above 3x" in g.load_library().gvtm_last_error()


@pytest.mark.parametrize("voice,rate,crate,steps", CONTROL_RATE_CASES, ids=lambda v: str(v))
def test_control_rates(voice, rate, crate, steps):
    plan = _plan(voice, None, rate, crate)
    assert plan.info.control_steps == steps == round(float(internal_rate(voice)) / crate)
    assert plan.info.control_rate == crate
    for f in range(9):
        assert plan.output_count(f) == _oracle_count(voice, rate, f, crate) <= plan.output_capacity(f), f


@pytest.mark.parametrize("voice", VOICES)
def test_launch_shapes_do_not_depend_on_the_voice(voice):
    """Chunk 60 (84 992 B of LDS) up to 256 utterances, chunk 56 (80 800 B) beyond: tests/test_capi_model5_float_cpu.py
    for the male voice."""
    lib = g.load_library(diagnostics=True)
    plan = _plan(voice, diagnostics=True)
    for batch, lds in ((1, 84992), (256, 84992), (257, 80800), (4096, 80800)):
        out = (ctypes.c_size_t * 3)()
        assert lib.gvtm_debug_launch_shape(plan._h, batch, 0, out) == 0
        assert out[0] == 1 and out[2] == lds, (batch, out[2])
    plan.close()
