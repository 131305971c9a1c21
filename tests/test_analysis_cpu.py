"""Spectrum analysis without a GPU: the names, the refusals, the window tables and the counts of the gvtm_analysis_* entries,
and gvtm_analysis_apply_host, the restatement the device is held to, against the numpy restatement of the rule
(tests/analysis_cases.py, which also gives the bars)."""
import os
import re

import numpy as np
import pytest

import analysis_cases as ac
import gama_tts_amd as g
from gama_tts_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gvtm_analysis_create", "gvtm_analysis_destroy", "gvtm_analysis_bin_count", "gvtm_analysis_window", "gvtm_analysis_buffer_count",
         "gvtm_analysis_reserve", "gvtm_analysis_apply_host", "gvtm_analyze_spectrum_device"]
WINDOWS = [(W, kind) for W in (32, 1024, 65536) for kind in (ac.BLACKMAN, ac.RECTANGULAR)]


def make(W=65536, kind=ac.BLACKMAN, log_scale=False, min_db=-120.0, max_freq=0.0, rate=44100):
    return g.Analysis(kind, W, log_scale, min_db, max_freq, rate, device=capi.DEVICE_NONE)


@pytest.fixture(scope="module")
def golden_audio():
    audio = ac.golden_track_audio()
    assert ac.N <= audio.size < 2 * ac.N
    return audio


def test_names_are_in_the_header_the_export_list_and_the_binding():
    header = open(os.path.join(ROOT, "include", "gama_vtm.h")).read()
    lib = g.load_library()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.PROTOTYPES and hasattr(lib, name), name
    for constant, value in [("GVTM_ANALYSIS_FFT_SIZE", 65536), ("GVTM_ANALYSIS_MAX_BINS", 32769), ("GVTM_WINDOW_RECTANGULAR", 0),
                            ("GVTM_WINDOW_TRIANGULAR", 1), ("GVTM_WINDOW_HANN", 2), ("GVTM_WINDOW_HAMMING", 3), ("GVTM_WINDOW_BLACKMAN", 4)]:
        assert re.search(r"#define\s+%s\s+%d\b" % (constant, value), header), constant
    assert (capi.ANALYSIS_FFT_SIZE, capi.ANALYSIS_MAX_BINS) == (65536, 32769)
    assert (capi.WINDOW_RECTANGULAR, capi.WINDOW_TRIANGULAR, capi.WINDOW_HANN, capi.WINDOW_HAMMING, capi.WINDOW_BLACKMAN) == (0, 1, 2, 3, 4)


@pytest.mark.parametrize("W,kind,rate", [(31, 4, 44100), (48, 4, 44100), (131072, 4, 44100), (1024, 5, 44100), (1024, -1, 44100), (1024, 4, 0)])
def test_bad_configurations_are_refused(W, kind, rate):
    with pytest.raises(capi.GvtmError) as refusal:
        make(W, kind, rate=rate)
    assert refusal.value.status == 1  # GVTM_ERR_INVALID_ARGUMENT


def test_device_entry_refuses_a_device_less_object():
    an = make(1024)
    counts, spectra = np.zeros(1, dtype=np.int64), np.zeros(an.n_bins, dtype=np.float32)
    with pytest.raises(capi.GvtmError) as refusal:
        an.analyze_device(np.zeros(ac.N, dtype=np.float32), ac.N, counts, 1, 1, d_spectra=spectra)
    assert refusal.value.status == 2  # GVTM_ERR_NO_DEVICE
    with pytest.raises(capi.GvtmError) as refusal:
        an.analyze_device(np.zeros(ac.N, dtype=np.float32), ac.N, counts, 1, 1)  # both outputs null: refused before that
    assert refusal.value.status == 1
    with pytest.raises(capi.GvtmError) as refusal:
        an.reserve(4)
    assert refusal.value.status == 2


@pytest.mark.parametrize("W", [32, 65536])
@pytest.mark.parametrize("kind", range(5))
def test_window_tables_equal_the_five_formulas_bit_for_bit(W, kind):
    assert np.array_equal(make(W, kind).window(), ac.window(kind, W))


@pytest.mark.parametrize("rate", [44100, 22050])
def test_bin_count_is_the_reference_loop(rate):
    on_a_bin = 100 * (float(rate) / 65536)  # exactly bin 100's frequency: `>` keeps it
    for max_freq in (100.0, 5000.0, rate / 2, on_a_bin, 0.0, -1.0, 1e9):
        assert make(1024, max_freq=max_freq, rate=rate).n_bins == ac.bin_count(rate, max_freq), max_freq
    assert ac.bin_count(rate, on_a_bin) == 101 and ac.bin_count(rate, 0.0) == 32769


def test_buffer_count():
    for span, want in [(65535, 0), (65536, 1), (131071, 1), (131072, 2), (3 * 65536 + 5, 3)]:
        for first in (0, 1, 12345):
            assert capi.analysis_buffer_count(first + span, first, 8) == want == ac.buffer_count(first + span, first, 8)
            assert capi.analysis_buffer_count(first + span, first, 1) == min(want, 1)
            assert capi.analysis_buffer_count(first + span, first, 0) == 0
    assert capi.analysis_buffer_count(100000, 100001, 4) == 0  # first > count
    assert capi.analysis_buffer_count(65536, 65536, 4) == 0
    assert capi.analysis_buffer_count(200000, -1, 4) == 0


def test_signal_view_is_the_normalised_samples_bit_for_bit(golden_audio):
    rng = np.random.default_rng(7)
    negative = rng.uniform(-0.5, 0.5, ac.N).astype(np.float32)
    negative[40000] = -0.8125 * 3  # the peak is negative
    late = rng.uniform(-0.01, 0.01, ac.N).astype(np.float32)
    late[60000] = 0.3  # the peak lies far behind a window of 32
    # the value edges of step 1: a sample that is no number (a NaN never becomes the peak, an infinity does), a peak whose
    # coefficient is inf or a denormal, and -0.0 only
    edges = {**ac.non_finite_cases(), **ac.extreme_peak_cases(), "minus-zero-only": ac.peak_position_cases()["minus-zero-only"]}
    for name, samples, W in [("negative-peak", negative, 1024), ("late-peak", late, 32), ("silence", np.zeros(ac.N, dtype=np.float32), 1024),
                             ("golden", golden_audio, 65536), ("golden", golden_audio, 32)] + [(name, s, ac.EDGE_W) for name, s in edges.items()]:
        _, signal, n = make(W).apply_host(samples, spectra=False)
        assert n == 1, name
        want = ac.normalised(samples[: ac.N])[:W]
        assert np.array_equal(signal[0].view(np.uint32), want.view(np.uint32)), name
    assert np.abs(ac.normalised(late)[:32]).max() < 0.05 and ac.normalised(negative).min() == -1.0
    # what the edges are, so that the table cannot lose them: the NaN behind the window changes nothing in front of it, the one
    # inside stays the only NaN; an infinite peak makes every finite sample a zero and itself a NaN; a denormal peak's
    # coefficient is inf, FLT_MAX's a denormal
    nan_behind, nan_inside = (ac.normalised(edges[name])[: ac.EDGE_W] for name in ("nan-behind", "nan-inside"))
    assert np.isfinite(nan_behind).all() and nan_behind.max() == 1.0
    assert np.flatnonzero(np.isnan(nan_inside)).tolist() == [100] and np.nanmax(nan_inside) == 1.0
    assert (ac.normalised(edges["inf-behind"])[: ac.EDGE_W] == 0).all()
    minus_inf = ac.normalised(edges["minus-inf-inside"])[: ac.EDGE_W]
    assert np.flatnonzero(np.isnan(minus_inf)).tolist() == [100] and (np.delete(minus_inf, 100) == 0).all()
    assert np.isinf(ac.normalised(edges["denormal"])).all()
    flt_max = ac.normalised(edges["flt-max"])
    assert 0.99 < flt_max.max() <= 1.0 and np.float32(1.0 / np.float64(np.finfo(np.float32).max)) < np.finfo(np.float32).tiny
    assert np.array_equal(ac.normalised(edges["minus-zero-only"]).view(np.uint32), np.full(ac.N, 0x80000000, dtype=np.uint32))


@pytest.mark.parametrize("W,kind", WINDOWS)
def test_linear_spectrum_of_the_host_entry_meets_the_bar(W, kind, golden_audio):
    an = make(W, kind)
    win = an.window()
    for name, (samples, first) in ac.inputs(W, golden_audio).items():
        buffers = 2 if name == "two-buffers" else 1
        spectra, signal, n = an.apply_host(samples, first, max_buffers=3)
        assert n == buffers and np.isnan(spectra[buffers:]).all() and np.isnan(signal[buffers:]).all(), name
        for k in range(buffers):
            buf = samples[first + k * ac.N: first + (k + 1) * ac.N]
            assert np.array_equal(signal[k], ac.normalised(buf)[:W]), name
            x = ac.prepared(buf, win)
            mag64 = ac.magnitudes64(x)
            limit, e32 = ac.bar(x, mag64)
            e = ac.error(spectra[k], mag64)
            print("W %5d window %d %-14s buffer %d: e %.3g, numpy float32 %.3g, bar %.3g" % (W, kind, name, k, e, e32, limit))
            assert e <= limit, (name, k, e, limit)


@pytest.mark.parametrize("W,kind", WINDOWS)
def test_an_empty_window_gives_exactly_zero_in_every_bin(W, kind):
    spectra, _, n = make(W, kind).apply_host(ac.empty_input(W))
    assert n == 1 and spectra.shape == (1, 32769) and (spectra == 0).all()
    log, _, _ = make(W, kind, log_scale=True, min_db=-20.0).apply_host(ac.empty_input(W))
    assert (log == np.float32(-20.0)).all()


@pytest.mark.parametrize("min_db", [-120.0, -20.0])
@pytest.mark.parametrize("W,kind", WINDOWS)
def test_log_spectrum_is_the_floored_logarithm_of_the_linear_one(W, kind, min_db, golden_audio):
    linear_object, log_object = make(W, kind, max_freq=5000.0), make(W, kind, log_scale=True, min_db=min_db, max_freq=5000.0)
    assert linear_object.n_bins == log_object.n_bins == ac.bin_count(44100, 5000.0) < 32769
    for name, (samples, first) in ac.inputs(W, golden_audio).items():
        linear, _, n = linear_object.apply_host(samples, first, max_buffers=2, signal=False)
        log, _, _ = log_object.apply_host(samples, first, max_buffers=2, signal=False)
        ac.check_log(log[:n], linear[:n], min_db)


def test_bins_are_cut_not_rescaled(golden_audio):
    """The bins below max_freq are the first bins of the whole spectrum."""
    whole, _, _ = make(1024).apply_host(golden_audio, signal=False)
    cut_object = make(1024, max_freq=5000.0)
    cut, _, _ = cut_object.apply_host(golden_audio, signal=False)
    assert cut.shape == (1, cut_object.n_bins) and np.array_equal(cut[0], whole[0, : cut_object.n_bins])
