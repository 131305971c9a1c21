"""What a plan fixes once for its float kernels (csrc/vtm_design.hpp: design_src_phase_table, static_wavetable), on
design-only plans of the diagnostics library.

The converter's coefficients by output phase: output sample ko reads the filter at frac = (ko * time_inc) & 0xFFFF, so
its 26 coefficients depend on ko mod P alone, P = 65536 / gcd(time_inc, 65536).  The host's table against a numpy float32
restatement of h + dh * (m / 256), the product rounded before the add, bit for bit over all phases, for several (internal
rate, output rate) pairs; and the plans that must have no table: P above the cap of 16384 phases (an odd time_inc has
65536), down-sampling, a double or mixed plan.

The static-wavetable flag: set for the shipped male voice, clear for a voice with tn_min != tn_max."""
import math

import numpy as np
import pytest

from gama_tts_amd import capi
from voice_cases import male_plan

CAP = 16384  # gvtm::kSrcPhaseCap
RECORD = 28  # gvtm::kSrcPhaseRecord: 13 + 13 coefficients and two pads
Z = 13       # zero crossings = taps per wing

# (SectionDelay, output rate) on the male voice -> (internal rate, time_inc, phases); the internal rate follows the SectionDelay
# (20034 Hz at 1, 40068 Hz at 2, 80137 Hz at 4)
TABLES = {
    (2, 44100.0): (40068, 59544, 8192),   # the benchmark's plan
    (1, 44100.0): (20034, 29772, 16384),  # exactly the cap
    (2, 48000.0): (40068, 54706, 32768),  # above it: see DECLINED
    (1, 22050.0): (20034, 59544, 8192),
    (2, 80136.0): (40068, 32768, 2),      # an exact 2:1: two phases
    (1, 32000.0): (20034, 41030, 32768),
}
HAVE = [k for k, v in TABLES.items() if v[2] <= CAP]
DECLINED = [k for k, v in TABLES.items() if v[2] > CAP]
ODD = (2, 44101.0)    # time_inc 59543: P = 65536
DOWN = (2, 32000.0)   # 40068 Hz in, 32 kHz out


def plan_of(delay, rate, precision=capi.PRECISION_F32, **overrides):
    return male_plan(overrides, rate=rate, delay=delay, precision=precision, diagnostics=True, device=capi.DEVICE_NONE)


def phases_of(time_inc):
    return 65536 // math.gcd(time_inc, 65536)


def restated(plan, phases):
    """h + dh * (m / 256) in float32 for every phase, both wings, from the plan's own float tables (widened in plan.table)."""
    h = plan.table(capi.TABLE_SRC_H).astype(np.float32)
    dh = plan.table(capi.TABLE_SRC_DH).astype(np.float32)
    assert h.shape == dh.shape == (Z * 256,)
    time_inc = int(plan.info.time_register_increment)
    frac = (np.arange(phases, dtype=np.int64) * time_inc) & 0xFFFF
    out = np.zeros((phases, RECORD), dtype=np.float32)
    taps = 256 * np.arange(Z)
    for wing, f in enumerate((frac, (~frac) & 0xFFFF)):
        idx = (f >> 8)[:, None] + taps[None, :]
        interp = ((f & 0xFF).astype(np.float32) / np.float32(256.0))[:, None]
        product = (dh[idx] * interp).astype(np.float32)  # rounded on its own
        out[:, wing * Z:(wing + 1) * Z] = h[idx] + product
    return out


def test_the_case_table_states_each_plans_own_numbers():
    for (delay, rate), (fs, time_inc, phases) in TABLES.items():
        plan = plan_of(delay, rate)
        assert (int(plan.info.internal_sample_rate), int(plan.info.time_register_increment)) == (fs, time_inc), (delay, rate)
        assert phases == phases_of(time_inc) and plan.info.upsampling, (delay, rate)
        plan.close()
    assert TABLES[(2, 44100.0)][2] == 8192 and HAVE and DECLINED


@pytest.mark.parametrize("delay,rate", HAVE)
def test_the_hosts_table_is_the_float32_restatement_bit_for_bit(delay, rate):
    plan = plan_of(delay, rate)
    phases = TABLES[(delay, rate)][2]
    assert plan.src_phases() == phases
    table = plan.src_phase_table()
    assert table.dtype == np.float32 and table.shape == (phases, RECORD)
    want = restated(plan, phases)
    assert np.array_equal(table.view(np.uint32), want.view(np.uint32))
    assert not table[:, 2 * Z:].any() and np.abs(table[:, 0]).max() > 0.5  # the pads; the centre tap of the first wing
    plan.force_generic_src()
    assert plan.src_phases() == 0 and plan.src_phase_table() is None
    plan.close()


@pytest.mark.parametrize("delay,rate", DECLINED + [ODD])
def test_a_plan_with_more_phases_than_the_cap_declines_the_table(delay, rate):
    plan = plan_of(delay, rate)
    time_inc = int(plan.info.time_register_increment)
    assert plan.info.upsampling and phases_of(time_inc) > CAP
    if (delay, rate) == ODD:
        assert time_inc % 2 == 1 and phases_of(time_inc) == 65536
    assert plan.src_phases() == 0 and plan.src_phase_table() is None
    plan.close()


def test_a_down_sampling_plan_has_no_table():
    plan = plan_of(*DOWN)
    assert not plan.info.upsampling
    assert plan.src_phases() == 0 and plan.src_phase_table() is None
    plan.close()


@pytest.mark.parametrize("precision", (capi.PRECISION_F64, capi.PRECISION_MIXED))
def test_a_double_or_mixed_plan_has_no_table(precision):
    plan = plan_of(2, 44100.0, precision)
    assert plan.src_phases() == 0
    plan.close()


def test_the_static_wavetable_flag_follows_the_voice():
    plan = plan_of(2, 44100.0)  # tests/golden/voice_male.txt
    assert plan.says_static_wavetable()
    plan.force_dynamic_wavetable()
    assert not plan.says_static_wavetable()
    plan.close()
    moving = plan_of(2, 44100.0, glottal_pulse_tn_min=16.0, glottal_pulse_tn_max=32.0)
    assert not moving.says_static_wavetable()
    moving.close()
    sine = plan_of(2, 44100.0, waveform=1, glottal_pulse_tn_min=16.0, glottal_pulse_tn_max=32.0)
    assert sine.says_static_wavetable()  # the sine never follows the amplitude, whatever tn_min and tn_max say
    sine.close()
