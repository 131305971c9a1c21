"""What tests/test_analysis_cpu.py and tests/test_gpu_analysis.py share: the numpy restatement of the analysis rule
(include/gama_vtm.h, "Spectrum analysis"; AnalysisWindow.cpp:189-361), the inputs, and the accuracy bars.

The bars.  A float DFT is held to the double DFT (numpy.fft.rfft in float64) of the exactly prepared floats x, by
e = max_i |mag - mag64| / max_i mag64.  The bar of a case is 8 x the e of numpy's own float32 transform of the same x (rfft of
a float32 array stays in single precision): the factor allows for another factorisation, the extra twiddle product of the
four-step split and the untangling pass.  The floor of the bar is 4 float ulps of the peak bin: that is the bar where numpy's
float32 transform is exact (e = 0: Nyquist alternation or DC under a rectangular window), and also where its e is not 0
but below what a float32 magnitude can hold at all -- a sinusoid on a bin under a rectangular window of 65 536 gives numpy
e = 6e-11 only because the double peak lies that close to a float, while half an ulp of that peak, the rounding of any
float32 result, is 6e-8 of it.  A buffer whose x is all zero has no peak to measure against: every bin must be exactly 0."""
import math

import numpy as np

N = 65536
BINS = N // 2 + 1
RECTANGULAR, TRIANGULAR, HANN, HAMMING, BLACKMAN = range(5)


def window(kind, W):
    """AnalysisWindow::setupWindow's five formulas in double, expression by expression, with this machine's libm cos
    (math.cos; numpy's own cos may differ from it in the last bit)."""
    i = np.arange(W, dtype=np.float64)

    def cos(a):
        return np.array([math.cos(v) for v in a], dtype=np.float64)

    if kind == RECTANGULAR:
        return np.ones(W)
    if kind == TRIANGULAR:
        center = (W - 1) / 2.0
        return 1.0 - np.abs((i - center) / center)
    coef = 2.0 * math.pi / (W - 1)
    if kind == HANN:
        return 0.5 * (1.0 - cos(coef * i))
    if kind == HAMMING:
        return 0.53836 - 0.46164 * cos(coef * i)
    if kind == BLACKMAN:
        alpha = 0.16
        a0, a1, a2 = (1.0 - alpha) / 2.0, 0.5, alpha / 2.0
        coef2 = 2.0 * coef
        return a0 - a1 * cos(coef * i) + a2 * cos(coef2 * i)
    raise ValueError(kind)


def bin_count(sample_rate, max_freq):
    """showData's loop: the first i whose plotX_[i] = i * freqCoef lies above maxFreq."""
    if max_freq <= 0:
        return BINS
    freq_coef = float(sample_rate) / N
    for i in range(BINS):
        if i * freq_coef > max_freq:
            return i
    return BINS


def buffer_count(count, first, max_buffers):
    return 0 if first > count else min(max_buffers, (count - first) // N)


def normalised(buf):
    """Step 1 on one buffer of 65 536 float32 samples."""
    buf = np.asarray(buf, dtype=np.float32)
    assert buf.shape == (N,)
    # the reference's loop is `if (absValue > maxValue) maxValue = absValue` from 0: a NaN is never greater, so it never becomes
    # the peak (np.abs(buf).max() would make it one); an infinity does, and the coefficient is then 0
    peak = np.fmax.reduce(np.abs(buf), initial=np.float32(0.0))
    if peak > 0:
        with np.errstate(over="ignore", invalid="ignore"):  # (a denormal peak's coefficient is inf; inf * 0 is NaN, as in C)
            return buf * np.float32(1.0 / np.float64(peak))
    return buf.copy()


def prepared(buf, win):
    """Step 3's x: the normalised samples under the window (a double product rounded to float), zeros behind."""
    x = np.zeros(N, dtype=np.float32)
    x[: win.size] = (normalised(buf)[: win.size].astype(np.float64) * win).astype(np.float32)
    return x


def magnitudes64(x):
    return np.abs(np.fft.rfft(x.astype(np.float64))) / 256.0


def bar(x, mag64):
    """(bar on e, numpy's own float32 e) for the prepared floats x, which are not all zero."""
    spectrum32 = np.fft.rfft(x)
    assert spectrum32.dtype == np.complex64
    mag32 = np.abs(spectrum32).astype(np.float64) / 256.0
    peak = mag64.max()
    e32 = float(np.abs(mag32 - mag64).max() / peak)
    floor = 4.0 * float(np.spacing(np.float32(peak))) / peak
    return max(8.0 * e32, floor), e32


def error(mag, mag64):
    return float(np.abs(mag.astype(np.float64) - mag64).max() / mag64.max())


def golden_track_audio():
    """A golden track's oracle output: the 2 s random track of tests/golden_cases.py at 44.1 kHz, 88 108 samples, so one buffer."""
    import golden_cases
    import oracle
    case = next(c for c in golden_cases.CASES if c["name"] == "rand1000_m0")
    return oracle.synthesize(oracle.male_config(44100.0, 1), golden_cases.track_for(case))


def inputs(W, golden_audio):
    """name -> (samples float32, first): the cases of the issue, the smallest that can still go wrong.  All but the last are
    one buffer from sample 0."""
    i = np.arange(N)
    rng = np.random.default_rng(20240 + W)

    def impulse(at, value=1.0):
        s = np.zeros(N, dtype=np.float32)
        s[at] = value
        return s

    def sinusoid(bins):
        return np.cos(2.0 * np.pi * bins * i / N).astype(np.float32)

    cases = {
        "impulse-0": impulse(0),
        "impulse-odd": impulse(7, -0.25),
        "impulse-last": impulse(W - 1),
        "dc": np.full(N, 0.5, dtype=np.float32),
        "sine-bin-1": sinusoid(1),
        "sine-bin-32767": sinusoid(32767),
        "sine-between": sinusoid(1000.5),
        "nyquist": np.where(i % 2 == 0, 1.0, -1.0).astype(np.float32),
        "noise": rng.standard_normal(N).astype(np.float32),
        "golden": np.asarray(golden_audio[:N], dtype=np.float32),
    }
    out = {name: (s, 0) for name, s in cases.items()}
    out["two-buffers"] = ((0.1 * rng.standard_normal(12345 + 2 * N + 100)).astype(np.float32), 12345)
    return out


def empty_input(W):
    """A buffer whose prepared x is all zero: an impulse behind the window, or (W = 65536) silence."""
    s = np.zeros(N, dtype=np.float32)
    if W < N:
        s[W] = 1.0
    return s


FIVE_COUNTS = [0, 65535, 65536, 140000, 200000]


def five_rows():
    """The ragged batch of test_gpu_analysis.py (its five_rows fixture, the same samples): five rows of one stride whose counts
    are FIVE_COUNTS; the samples behind a row's count are there and must not be read as buffers."""
    rng = np.random.default_rng(55)
    return [(0.3 * rng.standard_normal(FIVE_COUNTS[-1])).astype(np.float32) for _ in FIVE_COUNTS]


# ---- the float transform bit for bit (test_analysis_float_cpu.py, test_gpu_analysis_edges.py) ----

# every W at which the cut 2 n < W of analysis_input meets the column split n = 16 g + f + 128 n2 differently (W <= 256: inside
# one n2, the first g only up to 32; 512: two n2; above: many), under Blackman; and all five windows at 512
FLOAT_WINDOWS = [(W, BLACKMAN) for W in (32, 64, 128, 256, 512, 1024, 65536)] + [(512, kind) for kind in (RECTANGULAR, TRIANGULAR, HANN, HAMMING)]
# the inputs of inputs() the device is held to the host run of the same butterflies on
BITWISE_INPUTS = ("noise", "golden", "sine-between", "impulse-odd")


def ulp_distance(a, b):
    """The largest distance in float32 steps between two arrays of finite floats (0: the same bits, but for the sign of 0)."""
    def ordered(x):
        bits = x.view(np.int32).astype(np.int64)
        return np.where(bits < 0, -(bits & 0x7fffffff), bits)
    return int(np.abs(ordered(np.ascontiguousarray(a, dtype=np.float32)) - ordered(np.ascontiguousarray(b, dtype=np.float32))).max())


# ---- the value edges of step 1 (test_analysis_cpu.py, test_gpu_analysis_edges.py): one buffer each, W 1024, rectangular ----

EDGE_W = 1024
# a peak in every lane of a DPP row of analysis_peak_kernel: with 4-byte loads sample p is lane p mod 16 of its row
# (16 r + l), with 16-byte loads lane (p / 4) mod 16 (64 r + 4 l; 16 * 37 + l lies in the lanes 4 to 7); and the first and
# last sample of the window, of a thread's loop and of the buffer
PEAK_POSITIONS = [16 * 37 + l for l in range(16)] + [64 * 5 + 4 * l for l in range(16)] + [0, 63, 64, 1023, 1024, 4095, 4096, 65535]


def _quiet(seed=99):
    return np.random.default_rng(seed).uniform(-0.01, 0.01, N).astype(np.float32)


def peak_position_cases():
    """name -> buffer: noise of amplitude 0.01 with one sample of 0.75 at each of PEAK_POSITIONS; a negative peak; -0.0 only."""
    cases = {}
    for at in PEAK_POSITIONS:
        cases["peak-at-%d" % at] = _quiet()
        cases["peak-at-%d" % at][at] = 0.75
    cases["negative-peak"] = _quiet()
    cases["negative-peak"][16 * 37 + 9] = -0.75
    cases["minus-zero-only"] = np.full(N, -0.0, dtype=np.float32)
    return cases


def extreme_peak_cases():
    """name -> buffer whose peak is a float denormal (the coefficient overflows to inf), the smallest normal, FLT_MAX (the
    coefficient is a denormal), and 3e38 beside 1e38; the other samples are that peak times 0.1 to 0.9, either sign."""
    rng = np.random.default_rng(98)
    shape = (rng.uniform(0.1, 0.9, N) * rng.choice([-1.0, 1.0], N))
    cases = {}
    for name, peak in [("denormal", np.float32(1e-40)), ("tiny", np.finfo(np.float32).tiny), ("flt-max", np.finfo(np.float32).max), ("3e38", np.float32(3e38))]:
        buf = (shape * np.float64(peak)).astype(np.float32)
        buf[123] = peak
        if name == "3e38":
            buf[124] = np.float32(1e38)
        assert np.abs(buf).max() == peak and (buf != 0).all()
        cases[name] = buf
    return cases


def non_finite_cases():
    """name -> buffer of noise and a peak of 0.75 with one sample that is no number: behind or inside the window of EDGE_W."""
    cases = {}
    for name, at, value in [("nan-behind", 2000, np.nan), ("nan-inside", 100, np.nan), ("inf-behind", 2000, np.inf), ("minus-inf-inside", 100, -np.inf)]:
        buf = _quiet(97)
        buf[500] = 0.75
        buf[at] = value
        cases[name] = buf
    return cases


def check_log(out, linear, min_db):
    """A log spectrum against max(min_db, 20 log10(the linear output of the same object with log_scale = 0)): within 1e-4 dB
    (a float at 120 has an ulp of 7.6e-6: a few ulps and the logarithm's own error), exactly min_db wherever the linear value
    is 0 or below the floor.  (Within 1e-4 dB of the floor either side may have clamped.)"""
    with np.errstate(divide="ignore"):
        ref = 20.0 * np.log10(linear.astype(np.float64))
    below, above = ref < min_db - 1e-4, ref > min_db + 1e-4
    assert (out[below] == np.float32(min_db)).all()
    assert below[linear == 0].all()
    if above.any():
        assert np.abs(out[above].astype(np.float64) - ref[above]).max() <= 1e-4
    edge = ~(below | above)
    if edge.any():
        assert np.abs(out[edge].astype(np.float64) - np.maximum(ref[edge], min_db)).max() <= 1e-4
