"""Spectrum analysis on the device (gvtm_analyze_spectrum_device; csrc/vtm_analysis.hip) against the host entry
(gvtm_analysis_apply_host) and the bars of tests/analysis_cases.py: the signal view bit for bit, the linear spectrum within
the bar of the double DFT and within the sum of both bars of the host entry, the log spectrum as the floored logarithm of the
linear one.  Batches with utterances of no, one and two buffers, first samples that take the aligned and the unaligned loads,
rows behind an utterance's buffers that must keep their fill, slices over a scratch of one buffer, and the composition with
a synthesis entry on one stream with no synchronisation in between."""
import numpy as np
import pytest

import analysis_cases as ac
import gama_tts_amd as g
from gama_tts_amd import capi
import targets_cases
from device_io import current_stream, filled, to_device, to_host
from voice_cases import male_plan

pytestmark = pytest.mark.gpu

WINDOWS = [(W, kind) for W in (32, 1024, 65536) for kind in (ac.BLACKMAN, ac.RECTANGULAR)]


@pytest.fixture(scope="module")
def golden_audio():
    return ac.golden_track_audio()


def pair(W, kind, log_scale=False, min_db=-120.0, max_freq=0.0):
    """The same configuration as a device object and as a design-only one (the host entry's)."""
    return tuple(g.Analysis(kind, W, log_scale, min_db, max_freq, 44100, device=device) for device in (0, capi.DEVICE_NONE))


def run_device(an, rows, first, max_buffers, counts=None):
    """The device entry on `rows` (one float32 array per utterance, packed into rows of one stride) -> (spectra
    [B][max_buffers][n_bins], signal [B][max_buffers][W], buffers_out); the outputs start out NaN resp. -7."""
    batch, stride = len(rows), max(r.size for r in rows)
    audio = np.zeros((batch, stride), dtype=np.float32)
    for b, r in enumerate(rows):
        audio[b, : r.size] = r
    counts = np.asarray([r.size for r in rows] if counts is None else counts, dtype=np.int64)
    d_audio, d_counts = to_device(audio, counts)
    d_first = None if first is None else to_device(np.asarray(first, dtype=np.int64))[0]
    d_spectra = filled((batch, max_buffers, an.n_bins), np.nan, np.float32)
    d_signal = filled((batch, max_buffers, an.window_size), np.nan, np.float32)
    d_buffers = filled(batch, -7, np.int32)
    an.analyze_device(d_audio, stride, d_counts, batch, max_buffers, d_first, d_spectra, d_signal, d_buffers, current_stream())
    return to_host(d_spectra, d_signal, d_buffers)


def check_against_host(host, win, rows, first, max_buffers, spectra, signal, buffers, counts=None, label=""):
    """One batch's device outputs against the host entry and the bars; every figure is printed before anything about the
    spectra is asserted."""
    missed = []
    for b, samples in enumerate(rows):
        count = samples.size if counts is None else int(counts[b])
        f = 0 if first is None else int(first[b])
        n = capi.analysis_buffer_count(count, f, max_buffers)
        assert buffers[b] == n == ac.buffer_count(count, f, max_buffers), (label, b)
        assert np.isnan(spectra[b, n:]).all() and np.isnan(signal[b, n:]).all(), (label, b)  # the fill, untouched
        if n == 0:
            continue
        host_spectra, host_signal, host_n = host.apply_host(samples[:count], f, max_buffers)
        assert host_n == n
        assert np.array_equal(signal[b, :n].view(np.uint32), host_signal[:n].view(np.uint32)), (label, b)
        for k in range(n):
            x = ac.prepared(samples[f + k * ac.N: f + (k + 1) * ac.N], win)
            if not x.any():  # an empty window: exactly 0 in every bin, on both sides
                assert (spectra[b, k] == 0).all() and (host_spectra[k] == 0).all(), (label, b, k)
                continue
            whole64 = ac.magnitudes64(x)
            mag64, peak = whole64[: host.n_bins], whole64.max()  # (a cut spectrum is held to the whole spectrum's peak and bar)
            limit, e32 = ac.bar(x, whole64)
            e = float(np.abs(spectra[b, k].astype(np.float64) - mag64).max() / peak)
            to_host_entry = float(np.abs(spectra[b, k].astype(np.float64) - host_spectra[k]).max() / peak)
            print("%s row %d buffer %d: device e %.3g (%.2f of the bar %.3g; numpy float32 %.3g); to the host entry %.3g"
                  % (label, b, k, e, e / limit, limit, e32, to_host_entry))
            if e > limit or to_host_entry > 2 * limit:
                missed.append((label, b, k, e, to_host_entry, limit))
    assert not missed, missed


@pytest.mark.parametrize("W,kind", WINDOWS)
def test_linear_spectrum_and_signal_view_of_every_case(W, kind, golden_audio):
    device, host = pair(W, kind)
    cases = ac.inputs(W, golden_audio)
    names = list(cases) + ["empty"]
    rows = [cases[name][0] for name in cases] + [ac.empty_input(W)]
    first = [cases[name][1] for name in cases] + [0]
    spectra, signal, buffers = run_device(device, rows, first, 2)
    check_against_host(host, host.window(), rows, first, 2, spectra, signal, buffers, label="W %d window %d" % (W, kind))
    assert buffers[names.index("two-buffers")] == 2 and buffers[names.index("golden")] == 1
    assert (spectra[names.index("empty"), 0] == 0).all()  # an empty window: exactly 0 in every bin


@pytest.mark.parametrize("min_db", [-120.0, -20.0])
@pytest.mark.parametrize("W,kind", WINDOWS)
def test_log_spectrum_is_the_floored_logarithm_of_the_linear_one(W, kind, min_db, golden_audio):
    linear_object, _ = pair(W, kind, max_freq=5000.0)
    log_object, _ = pair(W, kind, True, min_db, 5000.0)
    assert log_object.n_bins == ac.bin_count(44100, 5000.0)
    cases = ac.inputs(W, golden_audio)
    rows = [s for s, _ in cases.values()] + [ac.empty_input(W)]
    first = [f for _, f in cases.values()] + [0]
    linear, _, buffers = run_device(linear_object, rows, first, 2)
    log, _, log_buffers = run_device(log_object, rows, first, 2)
    assert np.array_equal(buffers, log_buffers)
    for b in range(len(rows)):
        n = int(buffers[b])
        assert n >= 1 and np.isnan(log[b, n:]).all()
        ac.check_log(log[b, :n], linear[b, :n], min_db)
    assert (log[-1, 0] == np.float32(min_db)).all()


COUNTS = [0, 65535, 65536, 140000, 200000]


@pytest.fixture(scope="module")
def five_rows():
    rng = np.random.default_rng(55)
    return [(0.3 * rng.standard_normal(COUNTS[-1])).astype(np.float32) for _ in COUNTS]


@pytest.mark.parametrize("W,kind,max_freq", [(65536, ac.BLACKMAN, 0.0), (1024, ac.RECTANGULAR, 5000.0)])
@pytest.mark.parametrize("first", [None, [0, 0, 0, 1, 3001], [0, 0, 0, 2, 3002]], ids=["first-null", "first-odd", "first-even"])
def test_a_ragged_batch_and_its_slices(W, kind, max_freq, first, five_rows):
    """Five rows over one stride, counts 0 to 200 000 (samples behind a row's count are there and must not be read as
    buffers), at most two buffers each; then the same batch over a scratch of one buffer: the same bits."""
    device, host = pair(W, kind, max_freq=max_freq)
    spectra, signal, buffers = run_device(device, five_rows, first, 2, COUNTS)
    assert buffers.tolist() == [0, 0, 1, 2, 2]
    check_against_host(host, host.window(), five_rows, first, 2, spectra, signal, buffers, COUNTS, label="W %d first %s" % (W, first))
    device.reserve(1)
    sliced = run_device(device, five_rows, first, 2, COUNTS)
    for whole, cut in zip((spectra, signal, buffers), sliced):
        assert np.array_equal(whole.view(np.uint32), cut.view(np.uint32))
    device.reserve(3)  # (slices that end inside an utterance's pairs)
    sliced = run_device(device, five_rows, first, 2, COUNTS)
    for whole, cut in zip((spectra, signal, buffers), sliced):
        assert np.array_equal(whole.view(np.uint32), cut.view(np.uint32))


def test_one_output_or_none():
    device, _ = pair(1024, ac.BLACKMAN)
    rows = [np.ones(ac.N, dtype=np.float32)]
    d_audio, d_counts = to_device(rows[0].reshape(1, -1), np.asarray([ac.N], dtype=np.int64))
    with pytest.raises(capi.GvtmError) as refusal:
        device.analyze_device(d_audio, ac.N, d_counts, 1, 1, stream=current_stream())
    assert refusal.value.status == 1
    d_signal, d_spectra = filled((1, 1, 1024), np.nan, np.float32), filled((1, 1, device.n_bins), np.nan, np.float32)
    device.analyze_device(d_audio, ac.N, d_counts, 1, 1, d_signal=d_signal, stream=current_stream())
    device.analyze_device(d_audio, ac.N, d_counts, 1, 1, d_spectra=d_spectra, stream=current_stream())
    signal, spectra = to_host(d_signal, d_spectra)
    assert (signal == 1.0).all() and np.isfinite(spectra).all() and spectra[0, 0, 0] > 0
    d_buffers = filled(1, -7, np.int32)
    device.analyze_device(d_audio, ac.N, d_counts, 1, 0, d_buffers_out=d_buffers, stream=current_stream())  # max_buffers 0
    assert to_host(d_buffers)[0].tolist() == [0]


def test_analysis_follows_synthesis_on_one_stream_without_synchronisation():
    """gvtm_synthesize_targets_device, then the analysis of its audio rows and out_counts, both enqueued before anything
    is waited for; the result is the host entry's on the samples copied back."""
    plan = male_plan(precision=capi.PRECISION_F32)
    lo, hi = 1, 80000
    while lo < hi:  # the shortest step count that yields one full buffer (about 1.5 s)
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if plan.targets_output_count(mid) >= ac.N else (mid + 1, hi)
    n_steps = lo
    assert ac.N <= plan.targets_output_count(n_steps) < ac.N + 16
    batch = 3
    step_counts = [n_steps, n_steps - 1, n_steps + 977]  # the second falls short of a buffer
    lists = [l for seed in range(batch) for l in targets_cases.spoken_lists(max(step_counts), 40 + seed)]
    offsets, steps, values = capi.pack_targets(lists)
    stride = plan.targets_output_capacity(max(step_counts))
    d_offsets, d_steps, d_values, d_step_counts = to_device(offsets, steps, values, np.asarray(step_counts, dtype=np.int32))
    d_audio, d_counts = filled((batch, stride), 0.0, np.float32), filled(batch, -7, np.int64)
    device, _ = pair(65536, ac.BLACKMAN, True, -120.0, 5000.0)
    linear_device, linear_host = pair(65536, ac.BLACKMAN, False, -120.0, 5000.0)
    d_log, d_linear = (filled((batch, 1, device.n_bins), np.nan, np.float32) for _ in range(2))
    d_signal, d_buffers = filled((batch, 1, 65536), np.nan, np.float32), filled(batch, -7, np.int32)
    stream = current_stream()
    plan.synthesize_targets_device(d_offsets, len(lists), None, d_steps, d_values, d_step_counts, batch, max(step_counts), d_audio, stride, d_counts,
                                   None, None, stream)
    device.analyze_device(d_audio, stride, d_counts, batch, 1, None, d_log, d_signal, d_buffers, stream)
    linear_device.analyze_device(d_audio, stride, d_counts, batch, 1, None, d_linear, None, None, stream)
    audio, counts, log, linear, signal, buffers = to_host(d_audio, d_counts, d_log, d_linear, d_signal, d_buffers)
    assert buffers.tolist() == [1, 0, 1] and counts[1] < ac.N <= counts[0]
    assert np.abs(audio[0, : ac.N]).max() > 0
    check_against_host(linear_host, linear_host.window(), list(audio), None, 1, linear, signal, buffers, counts, label="composition")
    for b in (0, 2):
        ac.check_log(log[b], linear[b], -120.0)
    assert np.isnan(log[1]).all()
