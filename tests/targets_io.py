"""What the tests of the parameter-targets family share on the device: the one-shot entries (gvtm_synthesize_targets_device and
its _voices, _model5 and _model5_voices forms) and the stream pushes (gvtm_stream_push_targets and its three forms).  One
runner for the four one-shot entries, which picks the entry from the plan's family and from whether there is a voice id per
utterance; one session driver for the four pushes; the comparisons of a session with a one shot; the guard pattern the audio
buffers start as; and the CPU tests' call of an entry on host memory that is never dereferenced.  A new form of the family
adds a case table and, where it has an entry of its own, a row to the choice in run_targets: not a runner.

An utterance is 16 lists of (steps, values), as in targets_cases.py.  torch is imported inside the functions (device_io.py):
collecting the tests needs no GPU."""
import numpy as np
import pytest

import gama_tts_amd as g
from gama_tts_amd import capi
from device_io import current_stream, filled, to_device, to_host
from stream_targets_cases import slice_lists
from targets_cases import spoken_lists

GUARD = 0xA5  # every byte of the audio buffer before the call
INVALID_ARGUMENT = 1


def guard_behind_counts(audio, counts):
    """Is every sample behind a row's count (a row left out, count -1: the whole row) still the pattern?"""
    pattern = np.frombuffer(bytes([GUARD] * 4), dtype=np.uint32)[0]
    return all((audio[b, max(int(counts[b]), 0):].view(np.uint32) == pattern).all() for b in range(audio.shape[0]))


def at_own_index(voice_ids):
    """The utterances that the grouping (a stable sort by voice, one workgroup each) leaves at the workgroup of their own index."""
    return [b for w, b in enumerate(sorted(range(len(voice_ids)), key=lambda b: voice_ids[b])) if w == b]


# ---- the one-shot entries ----

def method_of(model5, voices):
    """The name of Plan's method for the entry of a family, with or without a voice id per utterance."""
    return "synthesize_targets%s%s_device" % ("_model5" if model5 else "", "_voices" if voices else "")


def run_targets(plan, utterances, step_counts, voice_ids=None, ids=None, max_steps=None, status=True, peaks=True, counts=True, doctor=None, fill=GUARD,
                steps_in=True):
    """The plan's family's entry, with a voice id per utterance if voice_ids is given, on `utterances` (16 lists each; with
    ids: the lists, and ids [B][16] into them) -> (audio float32 [B][stride] that started out as `fill` bytes, counts that
    started out -7, maxabs that started out 5.0, statuses that started out -9); an output not asked for keeps its fill.
    doctor(offsets, steps, values) may spoil the packed tables; steps_in=False leaves d_step_counts out: every utterance has
    max_steps steps."""
    lists = utterances if ids is not None else [l for u in utterances for l in u]
    batch = len(step_counts)
    offsets, steps, values = capi.pack_targets(lists)
    if doctor:
        doctor(offsets, steps, values)
    max_steps = max([int(s) for s in step_counts] + [0]) if max_steps is None else max_steps
    stride = plan.targets_output_capacity(max_steps) if voice_ids is None else plan.targets_voices_output_capacity(max_steps)
    # (no table is empty on the device: one spare entry each)
    d_offsets, d_steps, d_values, d_counts_in = to_device(offsets, np.concatenate([steps, np.zeros(1, np.int32)]),
                                                           np.concatenate([values, np.zeros(1, np.float32)]), np.asarray(step_counts, dtype=np.int32))
    d_ids = None if ids is None else to_device(np.asarray(ids, dtype=np.int32).reshape(batch, 16))[0]
    d_audio = filled((batch, stride * 4), fill, np.uint8)
    d_counts, d_maxabs, d_status = filled(batch, -7, np.int64), filled(batch, 5.0, np.float32), filled(batch, -9, np.int32)
    voices = () if voice_ids is None else to_device(np.asarray(voice_ids, dtype=np.int32))
    getattr(plan, method_of(plan.info.model5, voice_ids is not None))(
        d_offsets, len(lists), d_ids, d_steps, d_values, d_counts_in if steps_in else None, *voices, batch, max_steps, d_audio, stride,
        d_counts if counts else None, d_maxabs if peaks else None, d_status if status else None, current_stream())
    audio, out_counts, maxabs, statuses = to_host(d_audio, d_counts, d_maxabs, d_status)
    return audio.view(np.float32).reshape(batch, stride), out_counts, maxabs, statuses


def one_shot(plan, utterances, step_counts, voice_ids=None):
    """run_targets on whole utterances, none of them refused -> (samples per utterance, maxabs)."""
    audio, counts, maxabs, statuses = run_targets(plan, utterances, step_counts, voice_ids)
    assert not statuses.any()
    if voice_ids is None:
        assert [int(c) for c in counts] == [plan.targets_output_count(int(s)) for s in step_counts]
    else:
        assert [int(c) for c in counts] == [plan.targets_voice_output_count(v, int(s)) for v, s in zip(voice_ids, step_counts)]
    return [audio[b, : counts[b]].copy() for b in range(len(step_counts))], maxabs


# ---- the stream pushes ----

def push_of(stream):
    """The stream's push for its plan's family; the _voices form on a plan that can hold several."""
    plan = stream._plan
    return getattr(stream, "push_targets%s%s" % ("_model5" if plan.info.model5 else "", "_voices" if isinstance(plan, capi.VoicesPlan) else ""))


def session(stream, utterances, schedule, after_push=None, push=None):
    """Pushes schedule[i][b] steps of utterance b in push i through `push` (a bound Stream.push_targets* method, by default
    push_of(stream); the points of those steps, counted from the push's first), calls after_push(steps given so far per
    utterance) behind each, then finishes -> (samples per utterance, maxabs, the samples each push returned for utterance 0)."""
    push = push or push_of(stream)
    batch = len(utterances)
    done, outs, first = [0] * batch, [[] for _ in range(batch)], []
    for counts in schedule:
        given = [slice_lists(utterances[b], done[b], int(counts[b])) for b in range(batch)]
        got = push(given, np.asarray(counts, dtype=np.int32))
        for b in range(batch):
            outs[b].append(got[b])
            done[b] += int(counts[b])
        first.append(got[0].size)
        if after_push:
            after_push(done)
    tail, maxabs = stream.finish()
    return [np.concatenate(outs[b] + [tail[b]]) for b in range(batch)], maxabs, first


def same(got, got_maxabs, want, want_maxabs, what=None):
    """A session's samples and peaks against one_shot's, as bytes."""
    for b in range(len(want)):
        assert got[b].size == want[b].size and got[b].tobytes() == want[b].tobytes(), (what, b)
    assert np.asarray(got_maxabs).tobytes() == np.asarray(want_maxabs).tobytes(), what


def same_as_one_shot(got, got_maxabs, one_shot, what=None):
    """A session's samples, counts and peaks against run_targets' (audio [B][stride], counts, maxabs, ...), as bytes."""
    audio, counts, maxabs = one_shot[:3]
    assert [x.size for x in got] == [int(c) for c in counts[: len(got)]], what
    same(got, got_maxabs, [audio[b, : counts[b]] for b in range(len(got))], maxabs, what)


def refused_push_changes_nothing(plan, push_name, totals, seed0=50):
    """The body of the one-voice stream tests' test_a_refused_push_changes_nothing: a session of five spoken utterances of
    `totals` steps on a stream of `plan`, pushed through Stream.<push_name> and its C entry gvtm_stream_<push_name>.  Between
    the first push and the rest, a push refused for three utterances' statuses, one for a stride of 8 samples (the caller's
    totals make some utterance synthesize more than that then) and one for a null audio buffer leave the points held, the
    caller's buffers and, as the finished session's equality with the one shot shows, the device state as they were."""
    lib, entry = plan._lib, getattr(plan._lib, "gvtm_stream_" + push_name)
    utterances = [spoken_lists(t, seed0 + b) for b, t in enumerate(totals)]
    want, want_maxabs = one_shot(plan, utterances, totals)
    stream = g.Stream(plan, 5)
    stream_push = getattr(stream, push_name)
    outs = [[] for _ in range(5)]

    def push(counts):
        given = [slice_lists(utterances[b], done[b], counts[b]) for b in range(5)]
        for b, samples in enumerate(stream_push(given, np.asarray(counts, dtype=np.int32))):
            outs[b].append(samples)
            done[b] += counts[b]

    done = [0] * 5
    push([13, 13, 7, 25, 0])  # (steps pending in every utterance but the last)
    held = stream.targets_points().copy()
    # utterance 1: a value that is not finite; 2: a point at step == its count; 3: a count above max_steps
    counts = [100, 100, 100, 100, 100]
    given = [slice_lists(utterances[b], done[b], counts[b]) for b in range(5)]
    bad = [list(u) for u in given]
    bad[1][3] = ([5], np.float32([np.nan]))
    bad[2][5] = ([0, 100], np.float32([1.0, 2.0]))
    with pytest.raises(g.GvtmError) as refused:
        stream_push(bad, np.asarray([100, 100, 100, 101, 100], dtype=np.int32), max_steps=100)
    assert refused.value.status == INVALID_ARGUMENT and refused.value.statuses.tolist() == [0, 3, 4, 1, 0]
    assert stream.targets_points().tolist() == held.tolist()
    # a stride one sample short and a null audio buffer with samples due are refused the same way
    offsets, steps, values = capi.pack_targets([l for u in given for l in u])
    stride = stream.targets_capacity(100)
    audio, out_counts, statuses = np.zeros((5, stride), np.float32), np.zeros(5, np.int64), np.full(5, -1, np.int32)
    p = capi._ptr
    assert entry(stream._h, p(offsets), p(steps), p(values), None, 100, p(audio), 8, p(out_counts), p(statuses)) == INVALID_ARGUMENT
    assert b"audio_stride" in lib.gvtm_last_error() and not statuses.any()
    assert entry(stream._h, p(offsets), p(steps), p(values), None, 100, None, stride, p(out_counts), p(statuses)) == INVALID_ARGUMENT
    assert stream.targets_points().tolist() == held.tolist() and not audio.any()
    # the corrected push and the rest of the session: nothing was synthesized twice
    push(counts)
    push([t - d for t, d in zip(totals, done)])
    tail, maxabs = stream.finish()
    same([np.concatenate(outs[b] + [tail[b]]) for b in range(5)], maxabs, want, want_maxabs)
    with pytest.raises(g.GvtmError):
        stream_push(given, 100)  # finished


# ---- the CPU tests' call ----

def device_entry(plan, entry_name, voices, batch=2, null=None, n_lists=32, ids=False, stride=None, max_steps=8):
    """Status of the C entry `entry_name` (voices: it takes d_voice_ids) on a small (host-memory, never dereferenced) batch;
    null: an argument to leave out."""
    a = dict(offsets=np.zeros(33, np.int64), steps=np.zeros(2, np.int32), values=np.zeros(2, np.float32), audio=np.zeros((2, 65536), np.float32),
             voices=np.zeros(2, np.int32))
    ptr = {k: (None if k == null else v.ctypes.data) for k, v in a.items()}
    list_ids = np.zeros((2, 16), np.int32).ctypes.data if ids else None
    voice_ids = (ptr["voices"],) if voices else ()
    return getattr(plan._lib, entry_name)(plan._h, ptr["offsets"], n_lists, list_ids, ptr["steps"], ptr["values"], None, *voice_ids, batch, max_steps,
                                          ptr["audio"], 65536 if stride is None else stride, None, None, None, None)
