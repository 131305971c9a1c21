"""The float transform of csrc/vtm_analysis.hpp on the host (gvtm_debug_analysis_float_host of the diagnostics library: the
functions the kernels of csrc/vtm_analysis.hip call, run workgroup by workgroup and thread by thread over plain arrays), held
to the double DFT with the bars of tests/analysis_cases.py.  This is where the index arithmetic of the passes A, B and C runs
without a GPU; tests/test_gpu_analysis_edges.py then holds the device to this run bit for bit."""
import numpy as np
import pytest

import analysis_cases as ac
import gama_tts_amd as g
from gama_tts_amd import capi


def make(W, kind, max_freq=0.0):
    return g.Analysis(kind, W, False, -120.0, max_freq, 44100, device=capi.DEVICE_NONE, diagnostics=True)


@pytest.fixture(scope="module")
def golden_audio():
    return ac.golden_track_audio()


@pytest.mark.parametrize("W,kind", ac.FLOAT_WINDOWS)
def test_the_headers_transform_meets_the_bar_of_every_case(W, kind, golden_audio):
    an = make(W, kind)
    win = an.window()
    missed = []
    for name, (samples, first) in ac.inputs(W, golden_audio).items():
        for k in range(2 if name == "two-buffers" else 1):
            buf = samples[first + k * ac.N: first + (k + 1) * ac.N]
            spectrum = an.debug_float_host(buf)
            x = ac.prepared(buf, win)
            if not x.any():  # (an impulse on a zero of the triangular or the Hann window: no peak to measure against)
                assert (spectrum == 0).all(), (name, k)
                continue
            mag64 = ac.magnitudes64(x)
            limit, e32 = ac.bar(x, mag64)
            e = ac.error(spectrum, mag64)
            print("W %5d window %d %-14s buffer %d: e %.3g (%.2f of the bar %.3g; numpy float32 %.3g)" % (W, kind, name, k, e, e / limit, limit, e32))
            if not e <= limit:
                missed.append((name, k, e, limit))
    assert not missed, missed
    assert (an.debug_float_host(ac.empty_input(W)) == 0).all()  # an empty window: exactly 0 in every bin


@pytest.mark.parametrize("log_scale", [False, True])
def test_a_bin_that_is_no_number_is_the_one_quiet_nan(log_scale):
    """analysis_level: the sign of a NaN that the butterflies make or pass on is the lanes' choice (x86 makes ffc00000 of
    inf - inf, gfx950 7fc00000), so every NaN bin leaves as 7fc00000 -- from the float transform and from the host entry."""
    an = g.Analysis(ac.RECTANGULAR, ac.EDGE_W, log_scale, -90.0, 0.0, 44100, device=capi.DEVICE_NONE, diagnostics=True)
    cases = {**ac.extreme_peak_cases(), **ac.non_finite_cases()}
    for name in ("denormal", "nan-inside", "minus-inf-inside"):
        entry, _, _ = an.apply_host(cases[name], signal=False)
        for spectrum in (an.debug_float_host(cases[name]), entry[0]):
            assert (spectrum.view(np.uint32) == 0x7fc00000).all(), name


def test_the_hook_answers_with_the_first_bins_of_a_cut_spectrum_and_with_the_host_entry(golden_audio):
    """n_bins below 32 769 cuts, it does not rescale; the hook's peak and normalisation are the host entry's (a quiet buffer
    whose peak lies behind the window), and a log object's hook is still linear."""
    buf = 0.25 * golden_audio[: ac.N]
    whole, cut_object = make(1024, ac.HANN).debug_float_host(buf), make(1024, ac.HANN, 5000.0)
    assert cut_object.n_bins == ac.bin_count(44100, 5000.0)
    assert np.array_equal(cut_object.debug_float_host(buf), whole[: cut_object.n_bins])
    log_object = g.Analysis(ac.HANN, 1024, True, -20.0, 0.0, 44100, device=capi.DEVICE_NONE, diagnostics=True)
    assert np.array_equal(log_object.debug_float_host(buf), whole)
    host, _, _ = make(1024, ac.HANN).apply_host(buf, signal=False)
    x = ac.prepared(buf, make(1024, ac.HANN).window())
    mag64 = ac.magnitudes64(x)
    limit, _ = ac.bar(x, mag64)  # (each side within the bar of the double DFT, so within two bars of each other)
    assert np.abs(whole.astype(np.float64) - host[0]).max() <= 2 * limit * mag64.max()
