"""Pins parity_rules.py: the rules decide several hundred GPU tests at once.  No GPU needed."""
import numpy as np
import pytest

from parity_rules import TOL5, check_batch, check_model5, within

REF = np.linspace(-1.0, 1.0, 401, dtype=np.float32) ** 3 * np.float32(0.75)  # peak 0.75 at both ends, 0.0 in the middle
PEAK_AT, SMALL_AT = 400, 230


def _moved(at, by):
    got = REF.copy()
    got[at] = np.float32(np.float64(REF[at]) + by)
    return got


def _ulps(at, n):
    """Sample `at` n float32 steps away from zero."""
    got = REF.copy()
    for _ in range(n):
        got[at] = np.nextafter(got[at], np.float32(np.inf) * np.sign(got[at]))
    return got


@pytest.mark.parametrize("tol", [0.0, 1e-9, 1e-5])
def test_an_exact_match_passes_at_every_tolerance(tol):
    assert within(REF.copy(), REF, tol)


def test_one_float32_ulp_of_the_sample_passes_and_two_at_peak_fail():
    assert within(_ulps(SMALL_AT, 1), REF, 1e-9) and within(_ulps(PEAK_AT, 1), REF, 1e-9)
    assert not within(_ulps(PEAK_AT, 2), REF, 1e-9)


@pytest.mark.parametrize("tol", [1e-5, 1e-3])
@pytest.mark.parametrize("peak", [None, 3.0])
def test_the_bound_is_tol_times_peak(tol, peak):
    bound = tol * (0.75 if peak is None else peak)
    assert bound > 4 * 2.0 ** -24  # (four float32 ulps of the peak, 0.75: the ulp term decides nothing here)
    for at in (SMALL_AT, PEAK_AT):
        assert within(_moved(at, 0.9 * bound), REF, tol, peak) and within(_moved(at, -0.9 * bound), REF, tol, peak)
        assert not within(_moved(at, 1.1 * bound), REF, tol, peak) and not within(_moved(at, -1.1 * bound), REF, tol, peak)


def test_zero_tolerance_is_bit_identity():
    assert not within(_ulps(SMALL_AT, 1), REF, 0.0)
    assert not within(REF[:-1], REF, 0.0)


def test_all_zero_and_empty_references():
    zero = np.zeros(50, np.float32)
    assert within(zero.copy(), zero, 1e-9) and within(zero.copy(), zero, 0.0)
    tiny = zero.copy()
    tiny[3] = 1e-30
    assert not within(tiny, zero, 1e-9)  # nothing but zero is within 1e-9 of a peak of zero
    empty = np.zeros(0, np.float32)
    assert within(empty, empty, 1e-9) and within(empty, empty, 0.0)


def test_check_model5():
    check_model5(REF.copy(), REF)
    check_model5(_moved(SMALL_AT, 0.9 * TOL5 * 0.75), REF)
    with pytest.raises(AssertionError):
        check_model5(_moved(SMALL_AT, 3e-6 * 0.75), REF)
    check_model5(_moved(SMALL_AT, 3e-6 * 0.75), REF, peak=3.0)  # peak=: the utterance's, where ref is a part of it
    ref = REF[:200]
    flips = ref.copy()
    flips[:21] = np.nextafter(flips[:21], np.float32(2.0))  # one ulp each: far inside TOL5, but 89.5 % exact
    with pytest.raises(AssertionError):
        check_model5(flips, ref)
    flips[:1] = ref[:1]
    check_model5(flips, ref)  # 90 % exact
    check_model5(flips[:199], ref[:199])  # fewer than 200 samples: the share is not asked for
    with pytest.raises(AssertionError):
        check_model5(_ulps(PEAK_AT, 2), REF, bypass=True)  # bypass: the fp64 rule
    check_model5(_ulps(PEAK_AT, 1), REF, bypass=True)
    with pytest.raises(AssertionError):
        check_model5(REF[:-1], REF)


def _launch(outs, maxabs=None):
    """(audio, counts, maxabs) as a launch returns them, rows padded with zeros."""
    audio = np.zeros((len(outs), max(o.size for o in outs) + 3), np.float32)
    for b, o in enumerate(outs):
        audio[b, : o.size] = o
    peaks = [np.abs(o).max() if o.size else 0.0 for o in outs]
    return audio, np.array([o.size for o in outs]), np.array(peaks if maxabs is None else maxabs, np.float32)


@pytest.mark.parametrize("float_class", [False, True], ids=["double", "float"])
def test_check_batch_count_maxabs_and_empty_utterances(float_class):
    empty = np.zeros(0, np.float32)
    refs = [REF, empty, REF[:50]]
    check_batch(*_launch(refs), refs, float_class)
    audio, counts, maxabs = _launch(refs)
    with pytest.raises(AssertionError):  # a wrong count, the samples right
        check_batch(audio, counts + [0, 0, 1], maxabs, refs, float_class)
    with pytest.raises(AssertionError):  # a wrong maxabs
        check_batch(audio, counts, np.nextafter(maxabs, np.float32(1.0)), refs, float_class)
    with pytest.raises(AssertionError):  # an empty utterance has maxabs 0
        check_batch(audio, counts, maxabs + np.float32([0, 1e-3, 0]), refs, float_class)


def test_check_batch_holds_each_class_to_its_bar():
    one_ulp = _ulps(SMALL_AT, 1)
    with pytest.raises(AssertionError):  # float: bit identity
        check_batch(*_launch([REF, one_ulp]), [REF, REF], True)
    check_batch(*_launch([REF, one_ulp]), [REF, REF], False)
    check_batch(*_launch([_moved(SMALL_AT, 0.9 * TOL5 * 0.75)]), [REF], False)
    with pytest.raises(AssertionError):  # double: TOL5 of the peak
        check_batch(*_launch([_moved(SMALL_AT, 1.1 * TOL5 * 0.75)]), [REF], False)
    check_batch(*_launch([_moved(SMALL_AT, 1.1 * TOL5 * 0.75)]), [REF], False, peak=3.0)
    with pytest.raises(AssertionError):  # bypass: the fp64 rule
        check_batch(*_launch([_ulps(PEAK_AT, 2)]), [REF], False, bypass=True)
