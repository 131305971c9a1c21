"""What "equal enough" means in the parity tests, once (pinned by tests/test_parity_rules.py).

Precision -> tolerance of the models 0-4 (test_gpu_parity.py's docstring has the reasons): the fp64 path 1e-9 of the
utterance's peak, the mixed path north_star's 1e-5, the float path bit-identical.  Both sides are float32 samples, so a
double-level difference can still flip the rounding of a sample: a sample may also differ by one float32 ulp of itself.
Reference model 5 differences its float32 resampler output and multiplies by the output rate, which turns such a flip
into a few 1e-7 of peak (test_gpu_model5.py's docstring): check_model5."""
import numpy as np

from gama_tts_amd import capi

TOL = {capi.PRECISION_F64: 1e-9, capi.PRECISION_MIXED: 1e-5, capi.PRECISION_F32: 0.0}
TOL5 = 2e-6       # model 5: every sample within this of the utterance's peak ...
MIN_EXACT = 0.90  # ... and this share of the samples bit-identical (utterances of 200 samples and more)


def within(got, ref, tol, peak=None):
    """Every sample within max(tol * peak, one float32 ulp of the reference sample); peak=None: the reference's own.
    tol == 0.0: bit-identical.  An empty reference passes."""
    if tol == 0.0:
        return np.array_equal(got, ref)
    ref64 = ref.astype(np.float64)
    if peak is None:
        peak = np.abs(ref64).max() if ref.size else 0.0
    d = np.abs(got.astype(np.float64) - ref64)
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    return bool((d <= np.maximum(ulp, tol * max(float(peak), 1e-300))).all())


def largest_error_within(got, ref, tol):
    """A second, looser rule (the streams' and the events entry's oracle checks): the largest difference within
    tol * peak + one float32 ulp of the PEAK."""
    peak = np.abs(ref).max()
    return bool(np.abs(got.astype(np.float64) - ref).max() <= tol * peak + np.spacing(np.float32(peak)))


def peak_err(got, ref):
    """max|got - ref| / max|ref| (a per-sample relative error is meaningless at zero crossings)."""
    ref = ref.astype(np.float64)
    peak = np.abs(ref).max()
    if peak == 0:
        return float(np.abs(got).max())
    return float(np.abs(got.astype(np.float64) - ref).max() / peak)


def check_model5(got, ref, bypass=False, peak=None):
    """Asserts model 5's bar; in bypass mode (no difference filter) the fp64 bar of the other models.  An empty reference
    passes, as in within()."""
    assert got.shape == ref.shape
    if ref.size == 0:
        return
    ref64 = ref.astype(np.float64)
    peak = float(np.abs(ref64).max()) if peak is None else float(peak)
    d = np.abs(got.astype(np.float64) - ref64)
    if bypass:
        assert within(got, ref, 1e-9, peak), float(d.max() / max(peak, 1e-300))
    else:
        assert float(d.max()) <= TOL5 * max(peak, 1e-300), float(d.max() / max(peak, 1e-300))
        if got.size >= 200:
            assert float((got == ref).mean()) >= MIN_EXACT, float((got == ref).mean())


def check_batch(audio, counts, maxabs, refs, float_class, bypass=False, peak=None):
    """Asserts a model 5 launch against refs[b], the reference samples of utterance b: the count exact, the samples to the
    class's bar (float: bit-identical; double: check_model5 with bypass and peak) and maxabs the largest of them."""
    for b, ref in enumerate(refs):
        assert counts[b] == ref.size, (b, counts[b], ref.size)
        got = audio[b, : ref.size]
        if float_class:
            assert within(got, ref, TOL[capi.PRECISION_F32]), b
        else:
            check_model5(got, ref, bypass, peak)
        assert maxabs[b] == (np.abs(got).max() if ref.size else 0.0), b
