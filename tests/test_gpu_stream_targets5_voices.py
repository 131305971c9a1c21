"""Streams fed parameter targets under a mix of voices on model 5 plans (gvtm_stream_push_targets_model5_voices on a stream
of gvtm_stream_create_voices; vtm5_synth_kernel with the voices and the targets flag together on behalf of a stream,
csrc/vtm_kernels_m5tv.hip and csrc/vtm_kernels_m5ftv.hip).

The bar is the header's contract: for every voice v, the steps of an utterance of voice v pushed in any grouping and then
finished give, bit for bit in both classes, the samples, count and maxabs of one
gvtm_synthesize_targets_model5_voices_device call on the whole lists under voice v -- hence in the float class the
reference's interactive model byte for byte under all five voices (tests/golden/targets5_voices_golden.npz, and
targets5_golden.npz for the male voice), in the double class the reference to parity_rules.check_batch.

A workgroup holds one utterance, and under several voices the workgroup's index is not the utterance's: the batches are
ordered so that NO utterance sits at its workgroup's own index, the condition under which the address of the filters' sums
in the stream state matters.  The filters run from 3021 (male) to about 7050 samples (baby); every voice's sessions are cut
with its own N_v (stream_targets_voices_cases; test_stream_targets_voices_cpu.py holds them to what they must cover).

No batch is above 13 utterances, no utterance longer than 2 N_v + chunk + 5 steps (chunk: the class's longest)."""
import os

import numpy as np
import pytest

import gama_tts_amd as g
from gama_tts_amd import capi
import oracle
import stream_targets_cases as sessions
import stream_targets_voices_cases as sv
import targets5_cases as cases5
import targets5_voices_cases as cases
from parity_rules import check_batch
from targets_cases import spoken_lists
from targets_io import at_own_index, one_shot as one_voice_one_shot, run_targets as one_shot_voices, same_as_one_shot, session
from voice_cases import male_plan
from voice_files import VOICES

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT, UNSUPPORTED = 1, 4


@pytest.fixture(scope="module")
def fixtures():
    return (np.load(os.path.join(oracle.GOLDEN_DIR, "targets5_voices_golden.npz")), np.load(os.path.join(oracle.GOLDEN_DIR, "targets5_golden.npz")))


def fixture_case(fixtures, float_class, n, v, total):
    """-> (the 16 lists, the reference's samples) of the fixtures' case (voice v, total steps)"""
    if v == 0:
        return cases5.lists_of(total), fixtures[1][cases5.name(float_class, total)]
    return cases.lists_of(VOICES[v], total, n[v]), fixtures[0][cases.name(float_class, VOICES[v], total)]


def fixture_sessions(fixtures, float_class, rows, chunk):
    """The three sessions of stream_targets_voices_cases.model5_sessions on the five-voice plan in a forced shape.  Each is in
    lockstep per voice, which is what makes a stream launch the shape its plan forces (a ragged session launches index 0,
    whatever is forced: stream_launch).  Under every voice the first utterance walks the fixtures' lists of the case, the
    second other lists of as many steps.  Every utterance is held to the one-shot voices entry here
    -> [(samples, maxabs, the reference's samples)] of the fixtures' utterances"""
    plan = cases.voices_plan(float_class, device=0, rows=rows)
    n = [plan.targets_filter_length(v) for v in range(5)]
    ids = list(sv.MODEL5_IDS)
    assert not at_own_index(ids) and len(ids) <= 13 and set(ids) == set(range(5))
    stream = g.Stream(plan, len(ids), voice_ids=ids)
    held = []
    for name, (totals, pieces) in sv.model5_sessions(n, chunk, max(cases.CHUNKS[float_class])).items():
        schedule = sv.schedule_of(pieces)
        assert sv.in_lockstep_per_voice(schedule, ids)
        fixture_at = [ids.index(v) for v in range(5)]
        utterances, refs = [], {}
        for b, (v, total) in enumerate(zip(ids, totals)):
            if b in fixture_at:
                lists, refs[b] = fixture_case(fixtures, float_class, n, v, total)
            else:
                lists = spoken_lists(total, 900 + b)
            utterances.append(lists)
        if held:
            stream.reset()
        got, maxabs, _ = session(stream, utterances, schedule, push=stream.push_targets_model5_voices)
        want = one_shot_voices(plan, utterances, totals, ids)
        assert not want[3].any()
        same_as_one_shot(got, maxabs, want, (name, chunk))
        for b, (v, t) in enumerate(zip(ids, totals)):
            assert got[b].size == plan.targets_voice_output_count(v, t), (name, b)
        held += [(got[b], maxabs[b], refs[b]) for b in fixture_at]
    assert len(held) == 15
    return held


# ---- a. the float class in its two shapes: the reference's bytes under all five voices ----

@pytest.mark.parametrize("rows,chunk", [(1, 60), (2, 52)], ids=["chunk60", "chunk52"])
def test_float_class_sessions_are_the_references_bytes(fixtures, rows, chunk):
    assert cases.CHUNKS[True][rows - 1] == chunk
    for i, (samples, peak, ref) in enumerate(fixture_sessions(fixtures, True, rows, chunk)):
        assert samples.size == ref.size and samples.tobytes() == ref.tobytes(), i
        assert peak == (np.abs(ref).max() if ref.size else 0.0), i


# ---- b. the double class: the one-shot voices entry's bytes, the reference to its bar ----

def test_double_class_sessions_equal_the_one_shot_voices_entry(fixtures):
    held = fixture_sessions(fixtures, False, 1, 56)
    audio = np.zeros((len(held), max(max(ref.size, x.size) for x, _, ref in held)), np.float32)
    for b, (x, _, _) in enumerate(held):
        audio[b, : x.size] = x
    check_batch(audio, [x.size for x, _, _ in held], np.asarray([peak for _, peak, _ in held]), [ref for _, _, ref in held], False)


# ---- c. ragged and edge sessions ----

def ragged_schedule(n, ids):
    """Seven utterances under voices `ids`: push counts at 0, 1, 3, 4 and 5 around the granule of four; utterances 0, 2 and 3
    cross their own voice's window in one push; utterance 5 is never pushed.  No total is above N_v + 400."""
    schedule = [[13, 0, 61, 1, 0, 0, 4], [0, 7, 11, 300, 3, 0, 5], [n[ids[0]] + 1, 5, 0, 0, 1, 0, 3], [12, 0, 24, 59, 0, 0, 1],
                [0, 4, 1, n[ids[3]] - 1, 5, 0, 0], [60, 1, 0, 2, 4, 0, 4], [3, 3, n[ids[2]], 5, 400, 0, 1]]
    totals = [int(t) for t in np.sum(schedule, axis=0)]
    assert totals[5] == 0 and {0, 1, 3, 4, 5} <= {c for push in schedule for c in push}
    assert all(t <= n[v] + 400 for t, v in zip(totals, ids))
    return schedule, totals


@pytest.mark.parametrize("float_class", [True, False], ids=["float", "double"])
def test_ragged_sessions_a_refused_push_and_reset_voices(float_class):
    plan = cases.voices_plan(float_class, device=0)
    n = [plan.targets_filter_length(v) for v in range(5)]
    ids = [4, 2, 0, 3, 1, 4, 0]
    assert not at_own_index(ids)
    schedule, totals = ragged_schedule(n, ids)
    utterances = [spoken_lists(max(t, 1), 10 + b, wide=b == 3) for b, t in enumerate(totals)]
    want = one_shot_voices(plan, utterances, totals, ids)
    stream = g.Stream(plan, len(ids), voice_ids=ids)
    held = []

    def after_push(done):
        # the bounded log, each utterance under its own voice's N (the baby's the longest)
        held.append(stream.targets_points().tolist())
        for b, v in enumerate(ids):
            assert held[-1][b] <= sv.log_bound(utterances[b], done[b], n[v]), (b, done)
        if len(held) == 2:
            # a refused push (utterance 1: a value that is not finite) leaves the stream as found
            bad = [sessions.slice_lists(utterances[b], done[b], 8) for b in range(len(ids))]
            bad[1][3] = ([5], np.float32([np.nan]))
            with pytest.raises(g.GvtmError) as refused:
                stream.push_targets_model5_voices(bad, 8)
            assert refused.value.status == INVALID_ARGUMENT and refused.value.statuses.tolist() == [0, 3, 0, 0, 0, 0, 0]
            assert stream.targets_points().tolist() == held[-1]

    got, maxabs, _ = session(stream, utterances, schedule, after_push, push=stream.push_targets_model5_voices)
    same_as_one_shot(got, maxabs, want, "ragged")
    assert held[-1][5] == 0
    # reset_voices with the ids permuted: the next session runs under the new voices' filters; once more after a session
    # that was not finished
    for permuted in ([2, 4, 0, 3, 4, 1, 0], [2, 0, 4, 4, 1, 0, 3]):
        assert not at_own_index(permuted) and sorted(permuted) == sorted(ids)
        stream.reset(voice_ids=permuted)
        schedule, totals = ragged_schedule(n, permuted)
        utterances = [spoken_lists(max(t, 1), 30 + b) for b, t in enumerate(totals)]
        got, maxabs, _ = session(stream, utterances, schedule, push=stream.push_targets_model5_voices)
        same_as_one_shot(got, maxabs, one_shot_voices(plan, utterances, totals, permuted), tuple(permuted))
        if permuted[0] == 2:
            stream.reset(voice_ids=ids)
            stream.push_targets_model5_voices([sessions.slice_lists(u, 0, min(t, 77)) for u, t in zip(utterances, totals)], np.minimum(totals, 77).astype(np.int32))


# ---- d. refusals, and plans of one voice ----

def test_the_other_family_is_refused_and_a_one_voice_plan_is_the_one_voice_entry():
    lists = spoken_lists(700, 3)
    stream = g.Stream(male_plan(precision=capi.PRECISION_F32), 1)
    with pytest.raises(g.GvtmError) as e:
        stream.push_targets_model5_voices([sessions.slice_lists(lists, 0, 10)], 10)
    assert e.value.status == UNSUPPORTED and "gvtm_stream_push_targets_voices" in str(e.value)
    assert stream.targets_points().tolist() == [0]
    for float_class in (True, False):
        plan = cases.single_plan(float_class, "small_child", device=0)
        want, want_maxabs = one_voice_one_shot(plan, [lists], [700])
        outs = {}
        for name in ("push_targets_model5_voices", "push_targets_model5"):
            stream = g.Stream(plan, 1)
            pieces = [getattr(stream, name)([sessions.slice_lists(lists, first, count)], count)[0] for first, count in ((0, 13), (13, 300), (313, 387))]
            tail, maxabs = stream.finish()
            outs[name] = (np.concatenate(pieces + [tail[0]]).tobytes(), maxabs.tobytes())
        assert outs["push_targets_model5_voices"] == outs["push_targets_model5"] == (want[0].tobytes(), np.asarray(want_maxabs).tobytes())


# ---- e. the filters' sums live in the utterance's own block of the stream state ----

@pytest.mark.parametrize("float_class,rows", [(True, 1), (True, 2), (False, 1)], ids=["float-chunk60", "float-chunk52", "double-chunk56"])
def test_the_sums_are_kept_in_each_utterances_own_block(float_class, rows):
    """Under several voices the workgroup's index is not the utterance's, and a launch that kept the sums by the workgroup's
    index would still find them again, launch after launch, as long as the grouping stays what it is: the samples cannot show
    it.  The state can (gvtm_debug_stream_targets_sums): after every push utterance b's block holds, bit for bit, the sums a
    one-voice stream of b's voice holds after the same pushes of the same lists.  The pushes are in lockstep per voice, so
    the stream launches the forced shape: every unit and instantiation of the variant keeps its sums this way."""
    plan = cases.voices_plan(float_class, device=0, rows=rows)
    ids = [4, 2, 0, 3, 1, 4, 0]
    assert not at_own_index(ids)
    pushes = [[13, 5, 61, 4, 8, 13, 61], [300, 7, 11, 300, 3, 300, 11], [12, 64, 24, 60, 100, 12, 24]]
    assert sv.in_lockstep_per_voice(pushes, ids)
    totals = [int(t) for t in np.sum(pushes, axis=0)]
    utterances = [spoken_lists(t, 70 + b) for b, t in enumerate(totals)]
    stream = g.Stream(plan, len(ids), voice_ids=ids)
    alone = [g.Stream(cases.single_plan(float_class, VOICES[v], device=0, rows=rows), 1) for v in ids]
    done = [0] * len(ids)
    for counts in pushes:
        stream.push_targets_model5_voices([sessions.slice_lists(utterances[b], done[b], counts[b]) for b in range(len(ids))], np.asarray(counts, dtype=np.int32))
        sums = stream.targets_sums()
        for b, single in enumerate(alone):
            single.push_targets_model5([sessions.slice_lists(utterances[b], done[b], counts[b])], counts[b])
            assert sums[b].tobytes() == single.targets_sums()[0].tobytes(), (b, done[b], counts[b])
            done[b] += counts[b]
        assert sums.any(axis=1).all()
    assert len({sums[b].tobytes() for b in range(len(ids))}) == len(ids)
