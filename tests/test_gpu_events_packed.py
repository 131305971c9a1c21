"""Event lists in from host memory, packed samples out, on the device (gvtm_synthesize_events_packed_host*,
vtm_tracks_kernel<TrackSliceArgs>).

The kernel alone, through the diagnostics library's hook, on a slice from the middle of a batch's tables: frames, counts and
drift states against the chained tracks oracle, bit for bit, in the padded rows and in the packed frames, with the SENTINEL
pattern intact behind every count and in both guards.

The entry against gvtm_synthesize_events_chunks_device on the same plan (chunk_cases.synthesize_chunks): samples in
[offset[b], offset[b] + count[b]), counts, maxabs, frame offsets and drift states with array_equal, zero gaps, an untouched
tail; int16 samples and scales against gvtm_synthesize_packed_host_pcm16 fed frames_out; frames_out against
gvtm_generate_tracks_chunks_device.  Then staging limits (slices of four, of one, a limit one byte short), page-locked
buffers and the flush-overrun row of a down-sampling plan.

Every utterance has at most a few dozen frames (the ring's edges are 31, 32, 33, 63, 64, 65)."""
import functools

import numpy as np
import pytest

import gama_tts_amd as g
from gama_tts_amd import capi
import event_lists
from chunk_cases import (DIVERSE_TRACKS, GUARD_FRAMES, SENTINEL, VARIANT_TRACKS, boundary_list, chain_oracle, check_rows, generate_tracks_chunks,
                         list_with_frames, offset_tables, random_list, synthesize_chunks)
from device_io import to_device, to_host
from track_cases import fresh_drift, make_singable, product_config, used_drift
from voice_cases import configs, configs5
from voices5_float_cases import float_voices_plan

pytestmark = pytest.mark.gpu

OUT_OF_MEMORY = 5
OUT_SENTINEL = {np.dtype(np.float32): 7.0, np.dtype(np.int16): 12345}
TAIL = 64  # samples of sentinel behind the capacity the layout asks for
RING_EDGES = (0, 1, 2, 31, 32, 33, 63, 64, 65)


def round8(n):
    return (int(n) + 7) // 8 * 8


# ---- 1. the kernel alone

def sentinel_frames(n_frames):
    import torch
    return torch.full((n_frames * 16,), SENTINEL, dtype=torch.int32, device="cuda:0").view(torch.float32)


def slice_batch():
    """-> (utterances, ids, lo, hi): a batch whose utterances [lo, hi) are the slice -- the nine ring-edge counts, one
    utterance without chunks, one of [empty, one-event, list] and one list of 241 events -- with two utterances of three
    chunks in front of it and one behind."""
    L = random_list
    front = [[L(700, 9), L(701, 0), L(702, 5)], [L(703, 17)]]
    inside = [[list_with_frames(c)] for c in RING_EDGES] + [[], [L(704, 0), L(705, 1), list_with_frames(40)], [boundary_list(241, seed=3)]]
    utterances = front + inside + [[L(706, 12)]]
    ids = [b % 5 for b in range(len(utterances))]
    return utterances, ids, len(front), len(front) + len(inside)


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "rows-only"])
def test_slice_kernel_on_a_slice_from_the_middle_of_the_tables(packed):
    utterances, ids, lo, hi = slice_batch()
    n = hi - lo
    assert n % 2 == 0  # (an odd slice too: below)
    drift0 = used_drift(len(utterances))
    want = [chain_oracle(DIVERSE_TRACKS[v], u, drift0[b]) for b, (u, v) in enumerate(zip(utterances, ids))]
    counts = np.array([w[0].shape[0] for w in want])
    assert counts[lo: lo + 9].tolist() == list(RING_EDGES) and counts[lo + 9] == 0 and counts[lo + 10] == 40 and counts[hi - 1] > 600
    events, chunk_offsets, utt_chunks = offset_tables(utterances)
    event_base, event_end = int(chunk_offsets[utt_chunks[lo]]), int(chunk_offsets[utt_chunks[hi]])
    assert event_base > 0 and utt_chunks[lo] > 0 and event_end < events.shape[0]
    # the packed frames with one spare frame behind every utterance: what is written behind a count shows
    frame_offsets = np.concatenate([[0], np.cumsum(counts + 1)]).astype(np.int64)
    max_frames = int(counts[lo:hi].max())

    plan = g.VoicesPlan(configs(precision=capi.PRECISION_F32), 250.0, 0, diagnostics=True)
    plan.set_voice_tracks([product_config(c) for c in DIVERSE_TRACKS])
    # only the slice's events are on the device, at the front of their buffer
    d_events, d_chunk_offsets, d_utt_chunks, d_ids, d_drift, d_frame_offsets = to_device(
        events[event_base: event_end].view(np.uint8), chunk_offsets, utt_chunks[lo: hi + 1], np.asarray(ids[lo:hi], dtype=np.int32),
        np.ascontiguousarray(drift0[lo:hi]).copy(), frame_offsets[lo: hi + 1])
    rows = sentinel_frames(n * max_frames + GUARD_FRAMES)
    packed_frames = int(frame_offsets[hi] - frame_offsets[lo])
    d_packed = sentinel_frames(packed_frames + GUARD_FRAMES)
    d_counts, = to_device(np.full(n, 99, dtype=np.int32))
    rc = plan._lib.gvtm_debug_tracks_slice(plan._h, capi._ptr(d_events), event_base, capi._ptr(d_chunk_offsets), capi._ptr(d_utt_chunks), capi._ptr(d_ids),
                                           capi._ptr(d_frame_offsets) if packed else None, n, max_frames, capi._ptr(rows),
                                           capi._ptr(d_packed) if packed else None, capi._ptr(d_counts), capi._ptr(d_drift))
    assert rc == 0, plan._lib.gvtm_last_error()
    out, got_packed, got_counts, got_drift = to_host(rows, d_packed, d_counts, d_drift)
    got = (out[: n * max_frames * 16].reshape(n, max_frames, 16), out[n * max_frames * 16:], got_counts, got_drift)
    check_rows(got, want[lo:hi], max_frames, drift0[lo:hi], "slice")
    bits = got_packed.view(np.uint32).reshape(-1, 16)
    if not packed:
        assert (bits == SENTINEL).all()
        return
    for b in range(lo, hi):
        first = int(frame_offsets[b] - frame_offsets[lo])
        assert np.array_equal(bits[first: first + counts[b]], want[b][0].view(np.uint32)), b
        assert (bits[first + counts[b]: int(frame_offsets[b + 1] - frame_offsets[lo])] == SENTINEL).all(), b
    assert (bits[packed_frames:] == SENTINEL).all(), "written past the packed frames"


def test_slice_kernel_never_writes_at_or_beyond_the_next_utterances_frames():
    """An odd slice (the last workgroup holds one row) whose packed extents are shorter than two of its utterances: the
    frames stop at frame_offsets[b + 1], the padded rows, counts and drift states are those of the whole utterances."""
    utterances = [[list_with_frames(c)] for c in (40, 33, 65)]
    ids = [0, 1, 2]
    drift0 = used_drift(3, seed=9)
    want = [chain_oracle(DIVERSE_TRACKS[v], u, drift0[b]) for b, (u, v) in enumerate(zip(utterances, ids))]
    extents = [40, 32, 1]
    frame_offsets = np.concatenate([[0], np.cumsum(extents)]).astype(np.int64) + 1000  # (only differences count)
    events, chunk_offsets, utt_chunks = offset_tables(utterances)
    plan = g.VoicesPlan(configs(precision=capi.PRECISION_F32), 250.0, 0, diagnostics=True)
    plan.set_voice_tracks([product_config(c) for c in DIVERSE_TRACKS])
    d_events, d_chunk_offsets, d_utt_chunks, d_ids, d_drift, d_frame_offsets = to_device(
        events.view(np.uint8), chunk_offsets, utt_chunks, np.asarray(ids, dtype=np.int32), drift0.copy(), frame_offsets)
    rows, d_packed = sentinel_frames(3 * 65 + GUARD_FRAMES), sentinel_frames(sum(extents) + GUARD_FRAMES)
    d_counts, = to_device(np.full(3, 99, dtype=np.int32))
    rc = plan._lib.gvtm_debug_tracks_slice(plan._h, capi._ptr(d_events), 0, capi._ptr(d_chunk_offsets), capi._ptr(d_utt_chunks), capi._ptr(d_ids),
                                           capi._ptr(d_frame_offsets), 3, 65, capi._ptr(rows), capi._ptr(d_packed), capi._ptr(d_counts), capi._ptr(d_drift))
    assert rc == 0, plan._lib.gvtm_last_error()
    out, got_packed, got_counts, got_drift = to_host(rows, d_packed, d_counts, d_drift)
    check_rows((out[: 3 * 65 * 16].reshape(3, 65, 16), out[3 * 65 * 16:], got_counts, got_drift), want, 65, drift0, "cut")
    bits = got_packed.view(np.uint32).reshape(-1, 16)
    first = 0
    for b, extent in enumerate(extents):
        assert np.array_equal(bits[first: first + extent], want[b][0][:extent].view(np.uint32)), b
        first += extent
    assert (bits[first:] == SENTINEL).all()


# ---- 2. the entry against gvtm_synthesize_events_chunks_device

def singable(count):
    return make_singable(list_with_frames(count))


def entry_utterances():
    """0 to 3 chunks per utterance, empty and one-event chunks among them, every edge of the ring as an utterance's length or
    as a chunk boundary inside it; nine utterances (an odd batch)."""
    e0, e1 = event_lists.random_event_table(50, n_events=0), event_lists.random_event_table(51, n_events=1)
    return [[singable(31)], [], [singable(1), singable(32)], [singable(64)], [e0, e1, singable(33)], [singable(2)], [singable(20), singable(5), singable(9)],
            [singable(65)], [e1]]


def make_plan(kind):
    """-> (plan, ids or None for utterance b = b % voices)"""
    if kind in ("male-float", "male-fp64"):
        plan = g.VoicesPlan(configs(precision=capi.PRECISION_F32 if kind == "male-float" else capi.PRECISION_F64, names=["male"]), 250.0, 0)
        plan.set_voice_tracks([product_config(VARIANT_TRACKS[0])])
        return plan, False
    if kind == "male-22k":
        plan = g.VoicesPlan(configs(22050.0, 2, names=["male"]), 250.0, 0)
        plan.set_voice_tracks([product_config(VARIANT_TRACKS[0])])
        return plan, False
    plan = {"voices-float": lambda: g.VoicesPlan(configs(precision=capi.PRECISION_F32), 250.0, 0),
            "model5-double": lambda: g.VoicesPlan(configs5(), 250.0, 0), "model5-float": float_voices_plan}[kind]()
    plan.set_voice_tracks([product_config(c) for c in VARIANT_TRACKS])
    return plan, True


def run_entry(plan, utterances, ids, dtype, drift0, frames=True, pinned=False):
    """The entry into buffers pre-filled with sentinels, the samples' TAIL samples and the frames' GUARD_FRAMES frames longer
    than the layout asks for -> dict of out, offsets, frame_offsets, frames_out, counts, maxabs, scales, drift."""
    dtype = np.dtype(dtype)
    events, chunk_offsets, utt_chunks = plan.pack_event_lists(utterances)
    batch = len(utterances)
    want_frames, want_samples = plan.events_packed_layout(events, chunk_offsets, utt_chunks, ids)
    n_out, n_frames = int(want_samples[batch]) + TAIL, int(want_frames[batch]) + GUARD_FRAMES
    keep = []
    if pinned:
        keep = [g.PinnedArray(events.shape, capi.EVENT_DTYPE), g.PinnedArray((n_out,), dtype), g.PinnedArray((n_frames, 16), np.float32)]
        keep[0].array[...] = events
        events, out, frames_out = (k.array for k in keep)
    else:
        out, frames_out = np.empty(n_out, dtype), np.empty((n_frames, 16), np.float32)
    out[...] = OUT_SENTINEL[dtype]
    frames_out.view(np.uint32)[...] = SENTINEL
    r = dict(offsets=np.full(batch + 1, -1, np.int64), frame_offsets=np.full(batch + 1, -1, np.int64), counts=np.full(batch, -1, np.int64),
             maxabs=np.full(batch, -1.0, np.float32), scales=np.full(batch, -1.0, np.float32) if dtype == np.int16 else None,
             drift=None if drift0 is None else np.ascontiguousarray(drift0, dtype=np.float64).copy())
    plan.synthesize_events_packed_host_into(events, chunk_offsets, utt_chunks, out, ids, r["offsets"], r["frame_offsets"], frames_out if frames else None,
                                            r["counts"], r["maxabs"], r["scales"], r["drift"])
    assert np.array_equal(r["offsets"], want_samples) and np.array_equal(r["frame_offsets"], want_frames)
    r["out"], r["frames_out"] = out.copy(), frames_out.copy()
    for k in keep:
        k.close()
    return r


def assert_layout_kept(r):
    """every gap zero, the tail and the frames' guard untouched"""
    out, offsets, counts = r["out"], r["offsets"], r["counts"]
    for b in range(len(counts)):
        assert offsets[b] % 8 == 0 and offsets[b + 1] == round8(offsets[b] + counts[b]), b
        assert not out[offsets[b] + counts[b]: offsets[b + 1]].any(), b
    assert (out[offsets[-1]:] == OUT_SENTINEL[out.dtype]).all() and out.size == offsets[-1] + TAIL
    assert (r["frames_out"][r["frame_offsets"][-1]:].view(np.uint32) == SENTINEL).all()


def same_results(a, b, keys=None):
    """the same bytes (the guard behind frames_out is a NaN pattern: no comparison of values)"""
    for key in keys or a:
        assert (a[key] is None and b[key] is None) or (a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes()), key


@functools.lru_cache(maxsize=None)
def reference(kind, with_drift=True):
    """(plan, utterances, ids or None, initial drift states, gvtm_synthesize_events_chunks_device's results on the plan,
    gvtm_generate_tracks_chunks_device's)"""
    plan, mixed = make_plan(kind)
    utterances = [[singable(c)] for c in (19, 18, 3, 18, 0)] if kind == "male-22k" else entry_utterances()[: 4 if kind.startswith("model5") else None]
    batch = len(utterances)
    n_voices = 5 if mixed else 1
    ids = (np.arange(batch) % n_voices).astype(np.int32)
    drift0 = used_drift(batch, seed=11) if with_drift else fresh_drift(batch)
    frames = [sum(capi.tracks_frame_count(product_config(VARIANT_TRACKS[0]), capi.events_from_table(t)) for t in u) for u in utterances]
    max_frames = max(frames)
    assert max_frames <= 65
    stride = plan.voices_output_capacity(max_frames)
    ref = synthesize_chunks(plan, utterances, ids, max_frames, stride, drift0, entry=True)
    assert ref["frames"].tolist() == frames and ref["maxabs"].max() > 0.0
    tracks = generate_tracks_chunks(plan, utterances, ids, max_frames, drift0)
    return plan, utterances, ids if mixed else None, drift0, ref, tracks


def assert_entry_equals_reference(r, ref, tracks):
    counts, offsets = r["counts"], r["offsets"]
    assert np.array_equal(counts, ref["counts"]) and np.array_equal(r["maxabs"], ref["maxabs"])
    assert np.array_equal(np.diff(r["frame_offsets"]), ref["frames"])
    if r["drift"] is not None:
        assert np.array_equal(r["drift"], ref["drift"])
    for b in range(len(counts)):
        n, lo = int(counts[b]), int(offsets[b])
        if r["out"].dtype == np.float32:
            assert np.array_equal(r["out"][lo: lo + n], ref["audio"][b, :n]), b
        f0, f1 = int(r["frame_offsets"][b]), int(r["frame_offsets"][b + 1])
        assert np.array_equal(r["frames_out"][f0:f1].view(np.uint32), tracks[0][b, : f1 - f0].view(np.uint32)), b
    assert_layout_kept(r)


KINDS = ["male-float", "male-fp64", "voices-float", "model5-double", "model5-float"]


@pytest.mark.parametrize("dtype", [np.float32, np.int16], ids=["f32out", "pcm16"])
@pytest.mark.parametrize("kind", KINDS)
def test_entry_equals_the_device_entry(kind, dtype):
    plan, utterances, ids, drift0, ref, tracks = reference(kind)
    r = run_entry(plan, utterances, ids, dtype, drift0)
    assert_entry_equals_reference(r, ref, tracks)
    assert not np.array_equal(r["drift"], drift0)  # (the generators ran)
    if dtype == np.int16:
        # the packed entry fed the frames that came back
        n_frames = int(r["frame_offsets"][-1])
        pcm = np.full(r["out"].size, OUT_SENTINEL[np.dtype(np.int16)], np.int16)
        counts, maxabs, scales = np.full(len(utterances), -1, np.int64), np.full(len(utterances), -1.0, np.float32), np.full(len(utterances), -1.0, np.float32)
        plan.synthesize_packed_host_into(np.ascontiguousarray(r["frames_out"][:n_frames]), r["frame_offsets"], pcm, ids, None, counts, maxabs, scales)
        assert np.array_equal(pcm, r["out"]) and np.array_equal(scales, r["scales"]) and np.array_equal(counts, r["counts"])
        assert np.array_equal(maxabs, r["maxabs"]) and (scales[maxabs > 0] > 0).all() and pcm[: r["offsets"][-1]].any()


def test_without_drift_states_and_without_frames():
    plan, utterances, ids, drift0, ref, tracks = reference("male-float", with_drift=False)
    r = run_entry(plan, utterances, ids, np.float32, None)
    assert_entry_equals_reference(r, ref, tracks)
    bare = run_entry(plan, utterances, ids, np.float32, None, frames=False)
    assert (bare["frames_out"].view(np.uint32) == SENTINEL).all()
    same_results(bare, r, ("out", "offsets", "frame_offsets", "counts", "maxabs"))
    # a one-voice plan takes ids too (the voices launch): the same bytes
    with_ids = run_entry(plan, utterances, np.zeros(len(utterances), np.int32), np.float32, None)
    same_results(with_ids, r, ("out", "offsets", "frame_offsets", "frames_out", "counts", "maxabs"))
    # an empty batch
    assert plan._lib.gvtm_synthesize_events_packed_host(plan._h, None, None, None, None, 0, None, 0, None, None, None, 0, None, None, None) == 0


# ---- 3. slices

def set_bytes(plan, tables, width, frames_out=True):
    """The header's accounting of one staging set for a slice of these one-chunk utterances (one-voice plan)."""
    frame_counts = [capi.tracks_frame_count(product_config(VARIANT_TRACKS[0]), capi.events_from_table(t)) for t in tables]
    n, longest = len(tables), max(frame_counts)
    stride = round8(plan.voices_output_capacity(longest))
    aligned = sum(round8(plan.voice_output_count(0, f)) for f in frame_counts)
    events = (296 * sum(t.shape[0] for t in tables) + 63) // 64 * 64
    return events + 64 * n * longest + 4 * n * stride + width * aligned + (64 * sum(frame_counts) if frames_out else 0)




def test_staging_limit_slices_of_four_and_of_one():
    plan, _ = make_plan("male-float")
    tables = [singable(6)] * 32
    utterances = [[t] for t in tables]
    drift0 = used_drift(32, seed=13)
    unlimited = run_entry(plan, utterances, None, np.int16, drift0)
    assert plan.packed_stats().largest_slice == 32 and plan.packed_stats().slices == 1
    for per_slice in (4, 1):
        limit = 3 * set_bytes(plan, tables[:per_slice], 2)
        plan.set_staging_limit(limit)
        assert plan.packed_stats().staging_bytes <= limit  # what the call before left beyond it is gone
        limited = run_entry(plan, utterances, None, np.int16, drift0)
        st = plan.packed_stats()
        assert st.slices == 32 // per_slice >= 8 and st.largest_slice == per_slice and 0 < st.staging_bytes <= limit == st.limit
        same_results(limited, unlimited)
    assert_layout_kept(unlimited)


def test_staging_limit_ragged_and_one_byte_short():
    plan, _ = make_plan("male-float")
    counts = (3, 20, 0, 7, 12, 20, 1, 9, 16, 5, 2, 18)
    tables = [singable(c) for c in counts]
    utterances = [[t] for t in tables]
    drift0 = used_drift(len(counts), seed=14)
    unlimited = run_entry(plan, utterances, None, np.float32, drift0)
    longest = max(set_bytes(plan, [t], 4) for t in tables)
    plan.set_staging_limit(3 * longest)
    limited = run_entry(plan, utterances, None, np.float32, drift0)
    st = plan.packed_stats()
    assert st.slices >= 8 and 0 < st.staging_bytes <= st.limit == 3 * longest
    same_results(limited, unlimited)
    # one byte short of what the longest utterance needs: refused before any device work, nothing written
    plan.set_staging_limit(3 * longest - 1)
    events, chunk_offsets, utt_chunks = plan.pack_event_lists(utterances)
    batch = len(counts)
    out = np.full(unlimited["out"].size, 7.0, np.float32)
    frames_out = np.full((int(unlimited["frame_offsets"][-1]), 16), 7.0, np.float32)
    offsets, frame_offsets, got = np.full(batch + 1, -1, np.int64), np.full(batch + 1, -1, np.int64), np.full(batch, -1, np.int64)
    maxabs, drift = np.full(batch, -1.0, np.float32), drift0.copy()
    with pytest.raises(g.GvtmError) as err:
        plan.synthesize_events_packed_host_into(events, chunk_offsets, utt_chunks, out, None, offsets, frame_offsets, frames_out, got, maxabs, None, drift)
    assert err.value.status == OUT_OF_MEMORY and str(longest) in str(err.value)
    assert (out == 7.0).all() and (frames_out == 7.0).all() and (offsets == -1).all() and (frame_offsets == -1).all()
    assert (got == -1).all() and (maxabs == -1.0).all() and np.array_equal(drift, drift0)


# ---- 4. page-locked buffers, a down-sampling plan

def test_page_locked_buffers():
    plan, utterances, ids, drift0, ref, tracks = reference("male-float")
    pageable = run_entry(plan, utterances, ids, np.int16, drift0)
    pinned = run_entry(plan, utterances, ids, np.int16, drift0, pinned=True)
    same_results(pinned, pageable)
    assert_entry_equals_reference(pinned, ref, tracks)


def test_flush_overrun_row_of_a_down_sampling_plan():
    plan, utterances, ids, drift0, ref, tracks = reference("male-22k")
    assert plan.voice_output_count(0, 18) > plan.voice_output_count(0, 19)  # the shorter utterance is the longer row
    for dtype in (np.int16, np.float32):
        assert_entry_equals_reference(run_entry(plan, utterances, ids, dtype, drift0), ref, tracks)
