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
    peak = np.abs(buf).max()
    if peak > 0:
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
