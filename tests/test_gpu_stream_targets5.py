"""Streams fed parameter targets on model 5 plans (gvtm_stream_push_targets_model5): the session of the model the editor's
interactive window constructs, VocalTractModel5<T,1>(config, interactive = true), advancing a few steps at a time.

The bar is the header's contract: an utterance's steps pushed in any grouping and then finished give, bit for bit and in both
classes, the samples, count and maxabs of one gvtm_synthesize_targets_model5_device call on the whole lists -- hence in the
float class the reference's bytes (tests/golden/targets5_golden.npz), in the double class the reference to
parity_rules.check_batch.  The pieces sit around the granule of FOUR steps, the chunk of every shape of the kernel's targets
variant (float 60 / 52, double 56 / 24) and the filter length (3021); batches are in lockstep (the forced shapes) and ragged
(one utterance per workgroup); the log of points stays bounded; a refused push leaves the stream as it was; the feeds exclude
each other until a reset, after which a frames-fed session on the same stream is what it always was.

No utterance is longer than 3 N + 45 steps, no batch larger than 5.

The edge session (d.) has 3 N + 45 steps.  Three pieces of about a chunk's size do not fit it beside the three of the
window's size, so its cuts around the chunk are cuts in front of the steps chunk - 1, chunk and chunk + 1
(stream_targets5_cases.edge_pieces5_at_chunk); pieces of a chunk's size are those of a. and b."""
import os

import numpy as np
import pytest

import gama_tts_amd as g
from gama_tts_amd import capi
import oracle
import stream_targets5_cases as sessions5
import stream_targets_cases as sessions
import targets5_cases as cases
import tracks
from parity_rules import check_batch
from targets_io import one_shot, refused_push_changes_nothing, same, session
from voice_cases import configs5, male_plan, model5_plan

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT, UNSUPPORTED = 1, 4
N = cases.N
spoken_lists = cases.targets_cases.spoken_lists


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(oracle.GOLDEN_DIR, "targets5_golden.npz"))


def lockstep(pieces, batch):
    return [[p] * batch for p in pieces]


def against_fixture(fixture, float_class, got, maxabs, totals):
    """The sessions' samples against the reference's for the cases `totals`, by the class's bar."""
    refs = [fixture[cases.name(float_class, s)] for s in totals]
    audio = np.zeros((len(got), max(max(r.size for r in refs), max(x.size for x in got), 1)), np.float32)
    for b, x in enumerate(got):
        audio[b, : x.size] = x
    check_batch(audio, [x.size for x in got], maxabs, refs, float_class)


# ---- a. the float class: the reference's bytes, both shapes ----

@pytest.mark.parametrize("rows,chunk", [(1, 60), (2, 52)])
def test_float_class_pushes_are_the_references_bytes_in_both_shapes(fixture, rows, chunk):
    plan = model5_plan(rows=rows, float_class=True)
    assert plan.targets_filter_length() == N and cases.CHUNKS[True][rows - 1] == chunk
    total = 2 * N + chunk + 5
    lists = cases.lists_of(total)
    stream = g.Stream(plan, 1)
    got, maxabs, _ = session(stream, [lists], lockstep(sessions5.pieces5(chunk, N), 1))
    assert got[0].tobytes() == fixture[cases.name(True, total)].tobytes()
    assert got[0].size == plan.targets_output_count(total) and maxabs[0] == np.abs(got[0]).max()
    want, want_maxabs = one_shot(plan, [lists], [total])
    same(got, maxabs, want, want_maxabs)
    # the short cases one step at a time: only every fourth push launches, finish synthesizes the rest
    for total in (0, 1, 3, 4, 5, chunk + 1):
        stream.reset()
        got, maxabs, sizes = session(stream, [cases.lists_of(total)], lockstep([1] * total, 1))
        assert got[0].tobytes() == fixture[cases.name(True, total)].tobytes(), total
        assert got[0].size == plan.targets_output_count(total) and maxabs[0] == (np.abs(got[0]).max() if got[0].size else 0.0)
        assert [size > 0 for size in sizes] == [(i + 1) % 4 == 0 for i in range(total)]


# ---- b. the double class: the reference to its bar, the one-shot entry's bytes, both shapes ----

@pytest.mark.parametrize("rows,chunk,batch", [(1, 56, 1), (2, 24, 3)])
def test_double_class_pushes_equal_the_one_shot_in_both_shapes(fixture, rows, chunk, batch):
    plan = model5_plan(rows=rows)
    assert plan.targets_filter_length() == N and cases.CHUNKS[False][rows - 1] == chunk
    total = 2 * N + chunk + 5
    utterances = [cases.lists_of(total)] * batch  # (three in lockstep: the last workgroup of the two-utterance shape runs half empty)
    got, maxabs, _ = session(g.Stream(plan, batch), utterances, lockstep(sessions5.pieces5(chunk, N), batch))
    against_fixture(fixture, False, got, maxabs, [total] * batch)
    want, want_maxabs = one_shot(plan, utterances, [total] * batch)
    same(got, maxabs, want, want_maxabs)


# ---- c. ragged batches: one utterance per workgroup ----

@pytest.mark.parametrize("float_class", [True, False], ids=["float", "double"])
def test_ragged_batch_with_zeros_and_an_utterance_never_pushed(float_class):
    plan = model5_plan(float_class=float_class)
    schedule = [[13, 0, 61, 1, 0], [0, 7, 11, 300, 0], [N + 1, 5, 0, 0, 0], [12, 0, 24, 59, 0], [0, 0, 1, N - 1, 0], [60, 1, 0, 2, 0]]
    totals = [int(t) for t in np.sum(schedule, axis=0)]
    assert totals[4] == 0 and 0 in schedule[0][:4] and len(set(totals)) == 5
    utterances = [spoken_lists(max(t, 1), 10 + b, wide=b == 3) for b, t in enumerate(totals)]
    want, want_maxabs = one_shot(plan, utterances, totals)
    got, maxabs, _ = session(g.Stream(plan, 5), utterances, schedule)
    same(got, maxabs, want, want_maxabs)
    assert [x.size for x in got] == [plan.targets_output_count(t) for t in totals]


# ---- d. the edges of resuming, and the log ----

@pytest.mark.parametrize("float_class", [True, False], ids=["float", "double"])
def test_edges_of_resuming_and_the_bounded_log(float_class):
    plan = model5_plan(float_class=float_class)
    chunk = cases.CHUNKS[float_class][0]
    total = 3 * N + 45
    lists = sessions5.edge_lists5(N, total)
    pieces = sessions5.edge_pieces5_at_chunk(chunk, N, total)
    stream = g.Stream(plan, 1)
    held = []

    def after_push(done):
        # the points of the last N + 12 steps, and one more per list
        bound = sum(1 for steps, _ in lists for s in steps if done[0] - (N + 12) <= s < done[0]) + 16
        held.append(int(stream.targets_points()[0]))
        assert held[-1] <= bound, done

    got, maxabs, _ = session(stream, [lists], lockstep(pieces, 1), after_push)
    assert np.isfinite(got[0]).all() and maxabs[0] > 0 and maxabs[0] == np.abs(got[0]).max()
    want, want_maxabs = one_shot(plan, [lists], [total])
    same(got, maxabs, want, want_maxabs)
    assert len(held) == len(pieces) and held[-1] < sum(len(l[0]) for l in lists) // 2


# ---- e. a refused push leaves the stream as it was ----

def test_a_refused_push_changes_nothing():
    # (the stride of 8 samples is short: utterance 3 holds 125 steps then and synthesizes 124 of them)
    refused_push_changes_nothing(model5_plan(float_class=True), "push_targets_model5", [250, 200, 200, 200, 220])


# ---- f. feeds and plans ----

@pytest.mark.parametrize("float_class", [True, False], ids=["float", "double"])
def test_feeds_exclude_each_other_until_a_reset(float_class):
    plan = model5_plan(float_class=float_class)
    lists = spoken_lists(200, 60)
    params = tracks.random_tracks(1, 9, seed0=77, consonant_heavy=True)
    whole, counts, peak = plan.synthesize_host(params)
    stream = g.Stream(plan, 1)
    stream.push_targets_model5([sessions.slice_lists(lists, 0, 30)], 30)
    with pytest.raises(g.GvtmError) as e:
        stream.push(params[:, :4])
    assert e.value.status == INVALID_ARGUMENT and "targets" in str(e.value)
    assert int(stream.targets_points()[0]) > 0
    # after a reset a frames session on the same stream is what it always was: no stale sum, no stale mode
    stream.reset()
    assert int(stream.targets_points()[0]) == 0
    outs = [stream.push(params[:, :4])[0], stream.push(params[:, 4:])[0]]
    with pytest.raises(g.GvtmError) as e:
        stream.push_targets_model5([sessions.slice_lists(lists, 0, 30)], 30)
    assert e.value.status == INVALID_ARGUMENT and "frames" in str(e.value)
    tail, maxabs = stream.finish()
    frames_fed = np.concatenate(outs + [tail[0]])
    assert frames_fed.size == counts[0] and frames_fed.tobytes() == whole[0, : counts[0]].tobytes() and maxabs[0] == peak[0]
    # after a reset a targets session equals its own one shot
    stream.reset()
    want, want_maxabs = one_shot(plan, [lists], [200])
    got, maxabs, _ = session(stream, [lists], lockstep([30, 5, 150, 15], 1))
    same(got, maxabs, want, want_maxabs)
    # ... and another, cut elsewhere, after a session that was not finished
    stream.reset()
    stream.push_targets_model5([sessions.slice_lists(lists, 0, 77)], 77)
    stream.reset()
    got, maxabs, _ = session(stream, [lists], lockstep([1, 199], 1))
    same(got, maxabs, want, want_maxabs)


def test_unsupported_plans():
    offsets, steps, values = capi.pack_targets(spoken_lists(10, 0) * 2)
    voices = g.VoicesPlan(configs5(names=["male", "female"]), 250.0, 0)
    for stream in (g.Stream(voices, 2, voice_ids=[0, 1]), g.Stream(male_plan(precision=capi.PRECISION_F32), 2)):
        stride = stream.targets_capacity(10)
        audio, counts = np.zeros((2, stride), np.float32), np.zeros(2, np.int64)
        rc = stream._lib.gvtm_stream_push_targets_model5(stream._h, capi._ptr(offsets), capi._ptr(steps), capi._ptr(values), None, 10, capi._ptr(audio), stride,
                                                         capi._ptr(counts), None)
        assert rc == UNSUPPORTED and b"gvtm_stream_push_targets" in stream._lib.gvtm_last_error()
        assert stream.targets_points().tolist() == [0, 0]
