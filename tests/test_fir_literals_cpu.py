"""The float decimator's coefficients that the float kernels hold as literals (csrc/vtm_design.hpp: kGlottalFirF32) against
the filter a float plan designs, bit for bit, on design-only plans: every voice file of tests/golden/ at 44.1 and 48 kHz (the
design takes no argument, so they all design the same 47 floats), and that such plans say they use the table.  A double or
mixed plan, whose kernels read their 49 coefficients from LDS, says it does not."""
import numpy as np
import pytest

import gama_tts_amd as g
from gama_tts_amd import capi
from voice_files import VOICES, voice_path


def plan_of(voice, rate, precision=capi.PRECISION_F32, delay=1):
    return g.Plan(g.config_from_dict(g.read_config_file(voice_path(voice)), rate, delay, precision), 250.0, capi.DEVICE_NONE,
                  diagnostics=True)


def test_the_table_is_47_finite_symmetric_floats():
    table = capi.fir_literal_table()
    assert table.dtype == np.float32 and table.shape == (47,) and np.isfinite(table).all()
    assert np.array_equal(table.view(np.uint32), table[::-1].view(np.uint32))  # linear phase: h[keep] .. h[1] .. h[keep]


@pytest.mark.parametrize("rate", (44100.0, 48000.0))
@pytest.mark.parametrize("voice", VOICES)
def test_a_float_plan_designs_the_table_bit_for_bit_and_uses_it(voice, rate):
    plan = plan_of(voice, rate)
    designed = plan.table(capi.TABLE_FIR)  # the float design, widened
    assert plan.info.fir_taps == 47 and designed.shape == (47,)
    assert np.array_equal(designed.astype(np.float32).astype(np.float64), designed)
    assert np.array_equal(designed.astype(np.float32).view(np.uint32), capi.fir_literal_table().view(np.uint32))
    assert plan.uses_fir_literals()
    plan.force_generic_fir()
    assert not plan.uses_fir_literals()
    plan.close()


@pytest.mark.parametrize("delay", (1, 2, 3, 4))
def test_every_section_delay_of_a_float_plan_uses_the_table(delay):
    plan = plan_of("male", 44100.0, delay=delay)
    assert plan.uses_fir_literals()
    plan.close()


@pytest.mark.parametrize("precision", (capi.PRECISION_F64, capi.PRECISION_MIXED))
def test_a_double_or_mixed_plan_does_not(precision):
    plan = plan_of("male", 44100.0, precision)
    assert plan.info.fir_taps == 49 and not plan.uses_fir_literals()
    plan.close()
