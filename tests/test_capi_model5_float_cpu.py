"""Host side of the float class of reference model 5 (gvtm_plan_create_model5_float: VocalTractModel5<float,1>) without a
GPU: a design-only plan derives what the class's constructors derive in float -- rate, driver loop, the converter's
increments and with them every output length -- serves the float resampler tables and has no CPU synthesis path; and
sinf_glibc (csrc/vtm_math.hpp), which the sine waveform needs on the device, is this machine's sinf on every float of
[2^-13, 2 pi].

The cosine's pinned range is not widened: model 5 calls cos on 2 pi f T with f the band-pass centre frequency (below half
the internal rate: < pi) and with f = 62.3371 / r + 320.204 Hz, r >= 5 mm, of the radiation impedance (at most 12 788 Hz at
an internal rate of at least 50 kHz: < 1.61), both inside the [2^-13, 3.2] tests/test_capi_cpu.py holds cosf_glibc to."""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import gama_tts_amd as g
from gama_tts_amd import capi
import golden_cases
import model5_cases as cases
import oracle
from voice_cases import model5_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


_plan = functools.partial(model5_plan, "male", float_class=True, device=capi.DEVICE_NONE)  # (overrides, rate, crate)


def test_entry_takes_f32_only_and_the_factory_entry_still_refuses_it():
    d = g.read_config_file(oracle.VOICE5_MALE)
    plan = _plan()
    assert plan.info.model5 == 1 and plan.info.precision == capi.PRECISION_F32 and plan.info.device == capi.DEVICE_NONE
    for precision in (capi.PRECISION_F64, capi.PRECISION_MIXED):
        with pytest.raises(g.GvtmError) as ei:
            g.Plan(g.config5_from_dict(d, 48000.0, precision), 250.0, capi.DEVICE_NONE, float_model5=True)
        assert ei.value.status == 1
    with pytest.raises(g.GvtmError) as ei:  # gvtm_plan_create_model5 is the factory's model 5: VocalTractModel5<double,1>
        g.Plan(g.config5_from_dict(d, precision=capi.PRECISION_F32), 250.0, capi.DEVICE_NONE)
    assert ei.value.status == 1 and "fp64 only" in str(ei.value)


@pytest.mark.parametrize("case", cases.MALE_FLOAT_CASES, ids=lambda c: c["name"])
def test_design_matches_the_reference_vectors(case, golden):
    m = cases.load(case["fixture"])["manifest"][case["name"]]
    tr = cases.track_for(case, golden)
    plan = _plan(case["overrides"], case["rate"], case["crate"])
    i = plan.info
    _, oracle_rate = oracle.synthesize5(cases.oracle_config(case), np.zeros((0, 16), np.float32), case["crate"])
    # (the oracle reports (int) (rate * 1000.0f), formed in float: the plan's rate must give exactly that figure)
    assert int(np.float32(i.internal_rate_hz) * np.float32(1000.0)) == round(oracle_rate * 1000.0)
    assert abs(i.internal_rate_hz - m["fs"]) < 2e-3 and i.internal_rate_hz == float(np.float32(i.internal_rate_hz))
    assert i.control_steps * tr.shape[0] == m["steps"]
    assert plan.output_count(tr.shape[0]) == m["n"]
    assert i.output_rate == case["rate"] and i.upsampling == int(case["rate"] >= m["fs"])


def test_output_count_of_the_random_vectors():
    plan = _plan()
    manifest = golden_cases.random_golden()["manifest"]
    for seed in (31, 32):
        assert plan.output_count(60) == manifest["m5f_s%d" % seed]["n"]


def test_output_counts_follow_the_float_converter_through_its_flush_overrun():
    """44.1 kHz, every length from 90 to 120 frames: the float oracle's count, with the overrun at 106 frames."""
    plan = _plan(rate=44100.0)
    cfg = oracle.male5_config(44100.0, 1)
    counts = {f: plan.output_count(f) for f in range(90, 121)}
    for f, n in counts.items():
        assert n == oracle.synthesize5(cfg, np.zeros((f, 16), np.float32))[0].size, f
    assert counts[106] - counts[105] == 924 and counts[107] - counts[106] == -571
    assert plan.output_capacity(120) >= max(counts.values())


def test_resampler_tables_are_the_float_tables():
    plan = _plan()
    h, dh = np.empty(3328, dtype=np.float32), np.empty(3328, dtype=np.float32)
    oracle.lib().vtmo_src_filter_f32(h.ctypes.data, dh.ctypes.data)
    assert np.array_equal(plan.table(capi.TABLE_SRC_H), h.astype(np.float64))
    assert np.array_equal(plan.table(capi.TABLE_SRC_DH), dh.astype(np.float64))
    with pytest.raises(g.GvtmError):  # no wavetable / FIR in model 5 (Rosenberg source)
        plan.table(capi.TABLE_FIR)


def test_rejections_and_no_cpu_path():
    with pytest.raises(g.GvtmError):
        _plan(rate=0.0)
    for key, value in (("vocal_tract_length", "25.0"),                              # internal rate below 50 kHz
                       ("glottal_pulse_tn_min", "30.0"), ("glottal_pulse_tp", "0.5"),  # RosenbergBGlottalSource's checks
                       ("glottal_noise_cutoff", "0.5"), ("frication_noise_cutoff", "40000"),  # Butterworth update() range
                       ("nasal_radius_4", "0"), ("mix_offset", "0")):
        with pytest.raises(g.GvtmError) as ei:
            _plan({key: value})
        assert ei.value.status == 1, key
    with pytest.raises(g.GvtmError):  # above 3x the internal rate
        _plan(rate=192000.0)
    with pytest.raises(g.GvtmError) as ei:
        _plan().synthesize_host(np.zeros((1, 2, 16), np.float32))
    assert ei.value.status == 2  # GVTM_ERR_NO_DEVICE


SINF_LOOP = r"""
#include <math.h>
#include <stdio.h>
#include <string.h>
int gvtm_debug_short_math(int kind, const double* x, size_t n, double* out);
int main(void)
{
	static double x[65536], y[65536];
	float lo = 0x1p-13f, hi = 6.2831855f; /* float(2 pi), what t * float(2 pi) reaches at t = 1 */
	unsigned a, b, u, bad = 0;
	unsigned long total = 0;
	memcpy(&a, &lo, 4);
	memcpy(&b, &hi, 4);
	for (u = a; u <= b; u += 65536) {
		unsigned n = b - u + 1 < 65536 ? b - u + 1 : 65536, i;
		for (i = 0; i < n; ++i) { unsigned v = u + i; float f; memcpy(&f, &v, 4); x[i] = f; }
		if (gvtm_debug_short_math(8, x, n, y) != 0) return 2;
		for (i = 0; i < n; ++i) {
			float want = sinf((float) x[i]), got = (float) y[i];
			if (memcmp(&want, &got, 4) != 0 && bad++ < 5) printf("x = %a: sinf %a, sinf_glibc %a\n", x[i], want, got);
		}
		total += n;
	}
	printf("%lu floats, %u differ\n", total, bad);
	return bad != 0;
}
"""


def test_sinf_glibc_is_this_machines_sinf_on_every_float_up_to_two_pi(tmp_path):
    """RosenbergBGlottalSource.h:139 calls std::sin on t * 2 pi, t in [0, 1]; below 2^-12 both return the argument."""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    src, exe = str(tmp_path / "sinf_loop.c"), str(tmp_path / "sinf_loop")
    with open(src, "w") as f:
        f.write(SINF_LOOP)
    libdir = os.path.dirname(g.library_path(True))
    subprocess.run([cc, "-std=c99", "-O2", "-ffp-contract=off", src, "-L" + libdir, "-lgama_vtm_diag", "-lm", "-Wl,-rpath," + libdir, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "0 differ" in r.stdout
    # and a few known values through the Python binding of the same hook
    lib = g.load_library(diagnostics=True)
    x = np.array([0.0, 2.0 ** -13, 0.5, np.float32(np.pi), np.float32(2 * np.pi)], dtype=np.float64)
    y = np.empty_like(x)
    assert lib.gvtm_debug_short_math(8, x.ctypes.data, x.size, y.ctypes.data) == 0
    assert y[0] == 0.0 and y[1] == 2.0 ** -13 and abs(y[2] - np.sin(0.5)) < 1e-7 and abs(y[4]) < 1e-6


def test_shapes_of_the_float_class_and_the_batch_size_that_picks_them():
    """Chunk 60 (84 992 B of LDS: one workgroup per compute unit) up to 256 utterances, chunk 56 (80 800 B <= 80 KB: two)
    beyond; a diagnostics plan forces either as rows 1 / rows 2.  The numbers follow from Offsets<> in float
    (csrc/vtm_kernel_m5.inc) and are what DESIGN.md 4b states; the queries answer from the function every launch asks."""
    lib = g.load_library(diagnostics=True)
    d = g.read_config_file(oracle.VOICE5_MALE)
    cfg = g.config5_from_dict(d, 48000.0, capi.PRECISION_F32)
    chunk60, chunk56 = 84992, 80800
    assert chunk56 <= 80 * 1024 < chunk60
    for forced, want in ((0, None), (1, chunk60), (2, chunk56)):
        plan = g.Plan(cfg, 250.0, capi.DEVICE_NONE, diagnostics=True, rows=forced, float_model5=True)
        if forced:
            assert lib.gvtm_debug_lds_bytes(plan._h, forced) == want
        for batch in (1, 256, 257, 512, 4096):
            out = (ctypes.c_size_t * 3)()
            assert lib.gvtm_debug_launch_shape(plan._h, batch, 0, out) == 0
            assert out[0] == 1 and out[2] == (want or (chunk60 if batch <= 256 else chunk56)), (forced, batch, out[2])
        plan.close()
