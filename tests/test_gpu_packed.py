"""The packed host entries on the device (gvtm_synthesize_packed_host*, gvtm_plan_set_staging_limit, gvtm_plan_reserve).

Every case runs a ragged batch through the packed entry and through the padded host entry of the same plan
(gvtm_synthesize_batch_host* with NULL ids, gvtm_synthesize_voices_host* with ids) and pins, with array_equal: utterance
b's samples in [offset[b], offset[b] + count[b]), the counts (also against the layout's), maxabs and scales; that every
gap up to the next start is zero; and that a buffer pre-filled with a sentinel is untouched beyond offset[batch].

The batches: frame counts 0..20 and the same reversed (neighbours of very different length, every count mod 8 on some
row); five voices interleaved, each over 0..20 frames (all eight residues on the female rows); a flush-overrun row that is
longer than the row of the slice's longest utterance; both classes of model 5; staging limits that force slices of four
utterances and of one, and one that the longest utterance cannot meet (GVTM_ERR_OUT_OF_MEMORY, nothing written);
page-locked buffers; and gvtm_plan_reserve in front of gvtm_synthesize_batch_device."""
import functools

import numpy as np
import pytest

import gama_tts_amd as g
from gama_tts_amd import capi
import tracks
from device_io import run_batch_device
from voice_cases import configs, male_plan, model5_plan, padded

pytestmark = pytest.mark.gpu

OUT_OF_MEMORY = 5
SENTINEL = {np.dtype(np.float32): 7.0, np.dtype(np.int16): 12345}
TAIL = 64  # samples of sentinel behind the capacity the layout asks for


@functools.lru_cache(maxsize=None)
def utterances_of(frame_counts, seed):
    pool = tracks.random_tracks(len(frame_counts), max(max(frame_counts), 1), seed0=seed, consonant_heavy=True)
    return [np.ascontiguousarray(pool[b, :f]) for b, f in enumerate(frame_counts)]


UP_AND_DOWN = tuple(range(21)) + tuple(reversed(range(21)))


def round8(n):
    return (int(n) + 7) // 8 * 8


def set_bytes(plan, frame_counts, width):
    """The header's accounting of one staging set for a slice of these utterances (one-voice plan)."""
    n, longest = len(frame_counts), max(frame_counts)
    stride = round8(plan._lib.gvtm_voices_output_capacity(plan._h, longest))
    aligned = sum(round8(plan.output_count(f)) for f in frame_counts)
    return 64 * n * longest + 64 * sum(frame_counts) + 4 * n * stride + width * aligned


def greedy_slices(plan, frame_counts, width, set_limit):
    """The header's rule restated: a slice takes utterances in order while its set stays within set_limit (the batches here
    are far below a machine-full) -> the slices' sizes."""
    sizes, lo = [], 0
    while lo < len(frame_counts):
        hi = lo + 1
        while hi < len(frame_counts) and set_bytes(plan, frame_counts[lo: hi + 1], width) <= set_limit:
            hi += 1
        sizes.append(hi - lo)
        lo = hi
    return sizes


def padded_reference(plan, utterances, ids, dtype):
    """The padded host entry on the same plan -> (rows, counts, maxabs, scales or None)."""
    params, frames = padded(utterances)
    pcm = np.dtype(dtype) == np.int16
    if ids is None:
        res = plan.synthesize_host_pcm16(params, frames) if pcm else plan.synthesize_host(params, frames)
    else:
        res = plan.synthesize_host_pcm16(params, ids, frames) if pcm else plan.synthesize_host(params, ids, frames)
    return res if pcm else res + (None,)


def run_packed(plan, utterances, ids, dtype, pinned=False):
    """The packed entry into a buffer pre-filled with a sentinel, TAIL samples longer than the layout asks for ->
    (out, offsets, counts, maxabs, scales or None)."""
    frames, fo = plan.pack_utterances(utterances)
    batch = len(utterances)
    want = plan.packed_sample_offsets(fo, ids)
    keep = []
    if pinned:
        keep = [g.PinnedArray(frames.shape, np.float32), g.PinnedArray((int(want[batch]) + TAIL,), dtype)]
        keep[0].array[...] = frames
        frames, out = keep[0].array, keep[1].array
    else:
        out = np.empty(int(want[batch]) + TAIL, dtype)
    out[...] = SENTINEL[np.dtype(dtype)]
    offsets = np.full(batch + 1, -1, np.int64)
    counts = np.full(batch, -1, np.int64)
    maxabs = np.full(batch, -1.0, np.float32)
    scales = np.full(batch, -1.0, np.float32) if np.dtype(dtype) == np.int16 else None
    plan.synthesize_packed_host_into(frames, fo, out, ids, offsets, counts, maxabs, scales)
    assert np.array_equal(offsets, want)
    result = out.copy()
    for k in keep:
        k.close()
    return result, offsets, counts, maxabs, scales


def assert_packed_equals_padded(plan, packed, reference, utterances, ids):
    out, offsets, counts, maxabs, scales = packed
    rows, ref_counts, ref_maxabs, ref_scales = reference
    batch = len(utterances)
    assert np.array_equal(counts, ref_counts) and np.array_equal(maxabs, ref_maxabs)
    assert maxabs.max() > 0.0 and out[: offsets[batch]].any()  # (there is sound to compare)
    if ref_scales is not None:
        assert np.array_equal(scales, ref_scales)
    for b in range(batch):
        n, lo = int(counts[b]), int(offsets[b])
        voice = 0 if ids is None else int(ids[b])
        assert n == plan._lib.gvtm_voice_output_count(plan._h, voice, utterances[b].shape[0]), b
        assert lo % 8 == 0 and offsets[b + 1] == round8(lo + n), b
        assert np.array_equal(out[lo: lo + n], rows[b, :n]), (b, voice, utterances[b].shape[0])
        assert not out[lo + n: offsets[b + 1]].any(), b  # the gap
    assert (out[offsets[batch]:] == SENTINEL[out.dtype]).all() and out.size == offsets[batch] + TAIL


@functools.lru_cache(maxsize=None)
def male_case(precision, dtype):
    """The first batch on the male voice: (plan, utterances, the padded entry's result, the packed entry's)."""
    plan = male_plan(precision=precision)
    utterances = utterances_of(UP_AND_DOWN, 4100)
    return plan, utterances, padded_reference(plan, utterances, None, dtype), run_packed(plan, utterances, None, dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.int16], ids=["f32out", "pcm16"])
@pytest.mark.parametrize("precision", [capi.PRECISION_F32, capi.PRECISION_F64], ids=["float", "fp64"])
def test_male_up_and_down(precision, dtype):
    plan, utterances, reference, packed = male_case(precision, dtype)
    assert_packed_equals_padded(plan, packed, reference, utterances, None)
    st = plan.packed_stats()
    assert st.limit == 0 and st.slices >= 1 and st.staging_bytes >= set_bytes(plan, [20], np.dtype(dtype).itemsize)


@pytest.mark.parametrize("precision", [capi.PRECISION_F32, capi.PRECISION_F64], ids=["float", "fp64"])
def test_five_voices_interleaved(precision):
    plan = g.VoicesPlan(configs(precision=precision), 250.0, 0)
    frame_counts = tuple(i // 5 for i in range(105))  # every voice takes 0..20 frames
    ids = (np.arange(105) % 5).astype(np.int32)
    female = [plan.voice_output_count(1, f) for f, v in zip(frame_counts, ids) if v == 1]
    assert sorted(set(c % 8 for c in female)) == list(range(8))
    utterances = utterances_of(frame_counts, 4200)
    reference = padded_reference(plan, utterances, ids, np.int16)
    assert_packed_equals_padded(plan, run_packed(plan, utterances, ids, np.int16), reference, utterances, ids)


def test_overrun_row_is_longer_than_the_longest_utterances():
    plan = male_plan(rate=22050.0, delay=2)
    frame_counts = (19, 18, 3, 18, 0)
    assert plan.output_count(18) > plan.output_count(19)
    utterances = utterances_of(frame_counts, 4300)
    reference = padded_reference(plan, utterances, None, np.int16)
    assert_packed_equals_padded(plan, run_packed(plan, utterances, None, np.int16), reference, utterances, None)


@pytest.mark.parametrize("float_class", [False, True], ids=["double", "float"])
def test_model5(float_class):
    plan = model5_plan("male", float_class=float_class)
    utterances = utterances_of((4, 0, 9, 1), 4400)
    reference = padded_reference(plan, utterances, None, np.float32)
    assert_packed_equals_padded(plan, run_packed(plan, utterances, None, np.float32), reference, utterances, None)


def test_one_voice_plan_takes_ids_and_an_empty_batch():
    plan = g.VoicesPlan(configs(precision=capi.PRECISION_F32, names=["female"]), 250.0, 0)
    utterances = utterances_of((5, 0, 12), 4500)
    ids = np.zeros(3, np.int32)
    reference = padded_reference(plan, utterances, ids, np.float32)
    assert_packed_equals_padded(plan, run_packed(plan, utterances, ids, np.float32), reference, utterances, ids)
    fo = np.zeros(1, np.int64)
    assert plan._lib.gvtm_synthesize_packed_host(plan._h, None, fo.ctypes.data, None, 0, None, 0, None, None, None) == 0


def test_staging_limit_uniform():
    plan = male_plan(precision=capi.PRECISION_F32)
    utterances = utterances_of((6,) * 40, 4600)
    unlimited = run_packed(plan, utterances, None, np.float32)
    assert plan.packed_stats().largest_slice == 40
    limit = 3 * set_bytes(plan, [6] * 4, 4)
    plan.set_staging_limit(limit)
    assert plan.packed_stats().staging_bytes <= limit  # what the unlimited call left beyond it is gone
    limited = run_packed(plan, utterances, None, np.float32)
    st = plan.packed_stats()
    assert st.slices >= 10 and st.largest_slice <= 4 and 0 < st.staging_bytes <= limit == st.limit
    for a, b in zip(limited, unlimited):
        assert np.array_equal(a, b)
    assert_packed_equals_padded(plan, limited, padded_reference(plan, utterances, None, np.float32), utterances, None)


def test_staging_limit_ragged():
    plan, utterances, reference, unlimited = male_case(capi.PRECISION_F32, np.int16)
    plan = male_plan(precision=capi.PRECISION_F32)  # (a plan of its own: the cached one keeps no limit)
    longest = set_bytes(plan, [20], 2)
    plan.set_staging_limit(3 * longest + 1)
    limited = run_packed(plan, utterances, None, np.int16)
    st = plan.packed_stats()
    sizes = greedy_slices(plan, list(UP_AND_DOWN), 2, longest)
    assert sizes.count(1) > len(sizes) // 2  # (most slices hold one utterance: what this limit is for)
    assert st.slices == len(sizes) and st.largest_slice == max(sizes) and 0 < st.staging_bytes <= st.limit
    for a, b in zip(limited, unlimited):
        assert np.array_equal(a, b)
    # a set that the longest utterance does not fit: refused before any device work
    plan.set_staging_limit(3 * longest - 1)
    frames, fo = plan.pack_utterances(utterances)
    out = np.full(int(unlimited[1][-1]) + TAIL, SENTINEL[np.dtype(np.int16)], np.int16)
    counts, maxabs, scales = np.full(42, -1, np.int64), np.full(42, -1.0, np.float32), np.full(42, -1.0, np.float32)
    with pytest.raises(g.GvtmError) as err:
        plan.synthesize_packed_host_into(frames, fo, out, None, None, counts, maxabs, scales)
    assert err.value.status == OUT_OF_MEMORY and str(longest) in str(err.value)
    assert (out == SENTINEL[np.dtype(np.int16)]).all() and (counts == -1).all() and (maxabs == -1.0).all() and (scales == -1.0).all()


def test_page_locked_buffers():
    plan, utterances, reference, pageable = male_case(capi.PRECISION_F32, np.int16)
    pinned = run_packed(plan, utterances, None, np.int16, pinned=True)
    for a, b in zip(pinned, pageable):
        assert np.array_equal(a, b)
    assert_packed_equals_padded(plan, pinned, reference, utterances, None)


def test_reserve_in_front_of_the_device_entry():
    params = tracks.random_tracks(6, 20, seed0=4700, consonant_heavy=True)
    frames = np.full(6, 20, np.int32)
    results = []
    for reserve in (True, False):
        plan = male_plan(precision=capi.PRECISION_F32)
        if reserve:
            plan.reserve(20)
            plan.reserve(3)  # (shorter: nothing to do)
        results.append(run_batch_device(plan, params, frames, plan.output_count(20)))
    assert np.array_equal(results[0][0], results[1][0]) and np.array_equal(results[0][1], results[1][1])
    assert results[0][0].any()
    male_plan(precision=capi.PRECISION_F64).reserve(20)  # no table to build: GVTM_OK
    model5_plan("male", float_class=True).reserve(20)
