"""The analysis kernels (csrc/vtm_analysis.hip) at their layout and value edges, through the diagnostics library:
  - the slot table of AnalysisArgs (gvtm_debug_analyze_slots): every buffer on the row its utterance's slot names, every other
    row untouched, the same bits over a sliced scratch;
  - the float transform bit for bit: the device's linear spectrum against gvtm_debug_analysis_float_host, the same functions of
    csrc/vtm_analysis.hpp run on the host (tests/test_analysis_float_cpu.py holds that run to the double DFT), at every
    window size at which the cut of the window meets the column split differently, under all five windows, at all four
    16-byte classes of a buffer's first sample and with an odd row stride;
  - the value edges of step 1 through the public entry: a peak in every lane of a DPP row under both load widths, peaks whose
    coefficient is inf or a denormal, samples that are no numbers.
Every comparison is of bits (uint32 views).  Whether a NaN is also the same NaN is asked in one place,
test_the_nans_are_the_same_nans."""
import numpy as np
import pytest

import analysis_cases as ac
import gama_tts_amd as g
from gama_tts_amd import capi
from device_io import current_stream, filled, to_device, to_host

pytestmark = pytest.mark.gpu
COUNTS = ac.FIVE_COUNTS


@pytest.fixture(scope="module")
def five_rows():
    return ac.five_rows()


@pytest.fixture(scope="module")
def golden_audio():
    return ac.golden_track_audio()


def pair(W, kind, log_scale=False, min_db=-120.0, max_freq=0.0):
    """The same configuration as a device object and as a design-only one, both of the diagnostics library."""
    return tuple(g.Analysis(kind, W, log_scale, min_db, max_freq, 44100, device=device, diagnostics=True) for device in (0, capi.DEVICE_NONE))


def analyse(an, rows, first, max_buffers, counts=None, spectra=True, slots=None, out_stride=None):
    """The device entry (or, with slots, gvtm_debug_analyze_slots) on `rows` packed into rows of one stride -> (spectra, signal,
    buffers_out); the outputs are [batch][max_buffers or out_stride] rows that start out NaN, buffers_out -7."""
    batch, stride = len(rows), max(r.size for r in rows)
    audio = np.zeros((batch, stride), dtype=np.float32)
    for b, r in enumerate(rows):
        audio[b, : r.size] = r
    counts = np.asarray([r.size for r in rows] if counts is None else counts, dtype=np.int64)
    d_audio, d_counts = to_device(audio, counts)
    d_first = None if first is None else to_device(np.asarray(first, dtype=np.int64))[0]
    per_row = max_buffers if slots is None else out_stride
    d_spectra = filled((batch, per_row, an.n_bins), np.nan, np.float32) if spectra else None
    d_signal = filled((batch, per_row, an.window_size), np.nan, np.float32)
    d_buffers = filled(batch, -7, np.int32)
    if slots is None:
        an.analyze_device(d_audio, stride, d_counts, batch, max_buffers, d_first, d_spectra, d_signal, d_buffers, current_stream())
    else:
        d_slots, = to_device(np.asarray(slots, dtype=np.int32))
        an.debug_analyze_slots(d_audio, stride, d_counts, batch, max_buffers, d_slots, out_stride, d_first, d_spectra, d_signal, d_buffers, current_stream())
    if not spectra:
        return (None,) + to_host(d_signal, d_buffers)
    return to_host(d_spectra, d_signal, d_buffers)


def same_bits(got, want, label, nans_as_bits=True):
    """Prints how far two float arrays are apart, then asserts that they are the same bits.  nans_as_bits=False: a NaN must
    stand where a NaN stands, whichever NaN; everything else is still compared as bits."""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    differ = got.view(np.uint32) != want.view(np.uint32)
    both_nan = differ & np.isnan(got) & np.isnan(want)
    numbers = np.isfinite(got) & np.isfinite(want)
    ulps = ac.ulp_distance(got[numbers], want[numbers]) if numbers.any() else 0
    print("%s: %d of %d words differ (%d of them NaN on both sides), the finite ones by at most %d ulp" % (label, differ.sum(), differ.size, both_nan.sum(), ulps))
    if both_nan.any():
        print("    the NaNs that differ: the device's %s, the host's %s" % tuple(
            sorted("%08x" % w for w in np.unique(side.view(np.uint32)[both_nan])[:4]) for side in (got, want)))
    if not nans_as_bits:
        differ &= ~both_nan
    assert not differ.any(), (label, int(differ.sum()), np.flatnonzero(differ.reshape(-1))[:8].tolist())


# ---- the slot table ----

SLOTS, OUT_STRIDE = [3, 0, 2, 1, 2], 4


def test_the_slot_table_places_every_buffer_and_leaves_every_other_row(five_rows):
    device, _ = pair(1024, ac.BLACKMAN)
    first = [0, 0, 0, 1, 3002]
    spectra, signal, buffers = analyse(device, five_rows, first, 2, COUNTS)
    assert buffers.tolist() == [0, 0, 1, 2, 2]
    for reserved in (None, 1, 3):  # the whole batch in one launch, a slice per pair, slices that end inside an utterance's pairs
        if reserved:
            device.reserve(reserved)
        slotted_spectra, slotted_signal, slotted_buffers = analyse(device, five_rows, first, 2, COUNTS, slots=SLOTS, out_stride=OUT_STRIDE)
        assert np.array_equal(slotted_buffers, buffers)
        for out, plain, name in ((slotted_spectra, spectra, "spectra"), (slotted_signal, signal, "signal")):
            assert out.shape[:2] == (5, OUT_STRIDE)
            for b in range(5):
                used = {SLOTS[b] + k: k for k in range(int(buffers[b]))}
                for row in range(OUT_STRIDE):
                    if row in used:
                        assert np.isfinite(plain[b, used[row]]).all()
                        assert np.array_equal(out[b, row].view(np.uint32), plain[b, used[row]].view(np.uint32)), (name, reserved, b, row)
                    else:
                        assert np.isnan(out[b, row]).all(), (name, reserved, b, row)


# ---- the float transform, bit for bit ----

@pytest.mark.parametrize("W,kind", ac.FLOAT_WINDOWS)
def test_linear_spectrum_is_the_host_run_of_the_headers_transform_bit_for_bit(W, kind, golden_audio):
    device, host = pair(W, kind)
    cases = ac.inputs(W, golden_audio)
    rows = [cases[name][0] for name in ac.BITWISE_INPUTS]
    spectra, _, buffers = analyse(device, rows, None, 1)
    assert buffers.tolist() == [1] * len(rows)
    for b, name in enumerate(ac.BITWISE_INPUTS):
        same_bits(spectra[b, 0], host.debug_float_host(rows[b]), "W %d window %d %s" % (W, kind, name))


@pytest.mark.parametrize("stride,first", [(ac.N + 4, [0, 1, 2, 3]), (ac.N + 1, None)], ids=["first-0-to-3", "odd-stride"])
def test_the_bits_do_not_depend_on_where_a_buffer_starts(stride, first):
    """Rows a multiple of 16 bytes apart with first = 0 .. 3: the four 16-byte classes, 8-byte loads on and off; and three rows
    an odd number of samples apart.  The same buffer on every row."""
    device, host = pair(1024, ac.BLACKMAN)
    buf = ac.inputs(1024, np.zeros(ac.N))["noise"][0]
    batch = 4 if first else 3
    rows = []
    for b in range(batch):
        row = np.full(stride, 9.0, dtype=np.float32)  # (what lies around the buffer is larger than its peak)
        f = first[b] if first else 0
        row[f: f + ac.N] = buf
        rows.append(row)
    counts = [(first[b] if first else 0) + ac.N for b in range(batch)]
    spectra, signal, buffers = analyse(device, rows, first, 1, counts)
    assert buffers.tolist() == [1] * batch
    want, want_signal = host.debug_float_host(buf), ac.normalised(buf)[:1024]
    for b in range(batch):
        same_bits(spectra[b, 0], want, "stride %d row %d" % (stride, b))
        same_bits(signal[b, 0], want_signal, "stride %d row %d signal" % (stride, b))


# ---- the value edges of step 1 ----

@pytest.mark.parametrize("first", [0, 1], ids=["16-byte-loads", "4-byte-loads"])
def test_a_peak_in_every_lane_of_a_row(first):
    """One batch, one row per case; a sample in front of the buffer (first = 1) or behind it that is larger than the peak and
    must not count.  The signal view is the numpy restatement's bit for bit: the peak was found wherever it lay."""
    device, _ = pair(ac.EDGE_W, ac.RECTANGULAR)
    cases = ac.peak_position_cases()
    rows = []
    for buf in cases.values():
        row = np.full(ac.N + 4, 5.0, dtype=np.float32)  # (rows a multiple of 16 bytes apart: `first` alone picks the loads)
        row[first: first + ac.N] = buf
        rows.append(row)
    _, signal, buffers = analyse(device, rows, [first] * len(rows), 1, [first + ac.N] * len(rows), spectra=False)
    assert buffers.tolist() == [1] * len(rows)
    wrong = [name for b, (name, buf) in enumerate(cases.items())
             if not np.array_equal(signal[b, 0].view(np.uint32), ac.normalised(buf)[: ac.EDGE_W].view(np.uint32))]
    assert not wrong, wrong


def edge_rows(cases):
    return [np.concatenate([buf, np.zeros(3, dtype=np.float32)]) for buf in cases.values()]


def test_peaks_whose_coefficient_is_inf_or_a_denormal():
    device, host = pair(ac.EDGE_W, ac.RECTANGULAR)
    cases = ac.extreme_peak_cases()
    spectra, signal, buffers = analyse(device, edge_rows(cases), None, 1, [ac.N] * len(cases))
    assert buffers.tolist() == [1] * len(cases)
    for b, (name, buf) in enumerate(cases.items()):
        _, host_signal, _ = host.apply_host(buf, spectra=False)
        # (which NaN stands where one must: test_the_nans_are_the_same_nans below)
        same_bits(signal[b, 0], host_signal[0], name + " signal against the host entry", nans_as_bits=False)
        same_bits(signal[b, 0], ac.normalised(buf)[: ac.EDGE_W], name + " signal against numpy", nans_as_bits=False)
        same_bits(spectra[b, 0], host.debug_float_host(buf), name + " spectrum against the host run of the float transform", nans_as_bits=False)
    assert np.isinf(signal[list(cases).index("denormal"), 0]).all() and np.isnan(spectra[list(cases).index("denormal"), 0]).all()
    for name in ("tiny", "flt-max", "3e38"):
        b = list(cases).index(name)
        # (FLT_MAX times its denormal coefficient is one ulp short of 1, on the host as on the device)
        assert 0.9999999 < signal[b, 0, 123] <= 1.0 and np.isfinite(spectra[b, 0]).all() and spectra[b, 0].max() > 0, name


def test_samples_that_are_no_numbers():
    device, host = pair(ac.EDGE_W, ac.RECTANGULAR)
    log_device, _ = pair(ac.EDGE_W, ac.RECTANGULAR, True, -90.0)
    cases = ac.non_finite_cases()
    names = list(cases)
    spectra, signal, buffers = analyse(device, edge_rows(cases), None, 1, [ac.N] * len(cases))
    log, _, _ = analyse(log_device, edge_rows(cases), None, 1, [ac.N] * len(cases))
    assert buffers.tolist() == [1] * len(cases)
    for b, (name, buf) in enumerate(cases.items()):
        _, host_signal, _ = host.apply_host(buf, spectra=False)
        # (which NaN stands where one must: test_the_nans_are_the_same_nans below)
        same_bits(signal[b, 0], host_signal[0], name + " signal against the host entry", nans_as_bits=False)
        same_bits(signal[b, 0], ac.normalised(buf)[: ac.EDGE_W], name + " signal against numpy", nans_as_bits=False)
        same_bits(spectra[b, 0], host.debug_float_host(buf), name + " spectrum against the host run of the float transform", nans_as_bits=False)
    # a NaN behind the window: the peak ignores it, and the buffer is the one without it
    clean = cases["nan-behind"].copy()
    clean[2000] = 0.0
    same_bits(spectra[names.index("nan-behind"), 0], host.debug_float_host(clean), "nan-behind against the buffer without it")
    ac.check_log(log[names.index("nan-behind")], spectra[names.index("nan-behind")], -90.0)
    # inside the window every bin is a NaN, under log too
    assert np.isnan(spectra[names.index("nan-inside"), 0]).all() and np.isnan(log[names.index("nan-inside"), 0]).all()
    assert np.isnan(spectra[names.index("minus-inf-inside"), 0]).all()
    # an infinite peak behind the window: coefficient 0, x all zero, every bin exactly 0, the floor under log
    assert (spectra[names.index("inf-behind"), 0] == 0).all() and (log[names.index("inf-behind"), 0] == np.float32(-90.0)).all()


NAN_CASES = ["denormal", "nan-inside", "minus-inf-inside"]


@pytest.mark.parametrize("name", NAN_CASES)
def test_the_nans_are_the_same_nans(name):
    """The rows of the two tests above that hold NaNs, compared as bits, NaNs included: signal against the host entry and
    numpy, spectrum against the host run of the float transform.

    This is what found that the transform's NaNs were the lanes' choice: before analysis_level made every NaN bin the one
    quiet NaN 7fc00000, each bin that was a NaN on one side was a NaN on the other, but with the other sign -- denormal 32 385
    of 32 769 words (the device's 7fc00000, the host's ffc00000: inf - inf in a butterfly), nan-inside 16 384 words (the
    device's ffc00000, the host's 7fc00000), minus-inf-inside 16 384 words (7fc00000 against ffc00000); no word that is a
    number differed, and the signal views were the same bits throughout (the NaN of -inf * 0 included).  IEEE 754 leaves the
    sign of a NaN result open, and the x86 and the gfx950 lanes choose differently."""
    device, host = pair(ac.EDGE_W, ac.RECTANGULAR)
    buf = {**ac.extreme_peak_cases(), **ac.non_finite_cases()}[name]
    spectra, signal, buffers = analyse(device, edge_rows({name: buf}), None, 1, [ac.N])
    assert buffers.tolist() == [1]
    _, host_signal, _ = host.apply_host(buf, spectra=False)
    missed = []
    for got, want, label in ((signal[0, 0], host_signal[0], "signal against the host entry"), (signal[0, 0], ac.normalised(buf)[: ac.EDGE_W], "signal against numpy"),
                             (spectra[0, 0], host.debug_float_host(buf), "spectrum against the host run of the float transform")):
        try:
            same_bits(got, want, name + " " + label)
        except AssertionError as e:
            missed.append(e.args[0])
    assert not missed, missed
