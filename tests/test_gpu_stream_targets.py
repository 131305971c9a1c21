"""Streams fed parameter targets (gvtm_stream_push_targets, gvtm_stream_targets_capacity, gvtm_stream_targets_points): the
interactive window as a session that advances a few steps at a time.

The bar is the header's contract: an utterance's steps pushed in any grouping and then finished give, bit for bit and in
every precision, the samples, count and maxabs of one gvtm_synthesize_targets_device call on the whole lists; in float that
is also the oracle's float class at control rate = internal rate on gvtm_targets_apply_host's frames.  The pieces sit around
the granule of 12 steps, the chunk and the filter length; batches are ragged (one utterance per workgroup) and in lockstep
(rows forced to 2 and 4); the log of points the stream keeps stays bounded; a refused push leaves the stream as it was.

The lists are spoken (targets_cases.spoken_lists).  No utterance is longer than about 3 N + chunk + 5 steps."""
import numpy as np
import pytest

import gama_tts_amd as g
from gama_tts_amd import capi
import oracle
import stream_targets_cases as sessions
import targets_cases as cases
from targets_io import one_shot, refused_push_changes_nothing, same, session
from voice_cases import configs, male_plan, model5_plan

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT, UNSUPPORTED = 1, 4
N, CHUNK = 1002, 144  # the float male plan's filter length and one-row chunk


def one_row_chunk(precision):
    """The chunk of the one-row shape, which a stream of one utterance (and every ragged one) launches."""
    plan = male_plan(precision=precision, rows=1)
    return int(plan._lib.gvtm_debug_chunk_length(plan._h, 1))


def lockstep_schedule(pieces, batch):
    return [[p] * batch for p in pieces]


def the_pieces(n, chunk, total):
    pieces = [1, 11, 12, 13, chunk - 1, chunk, chunk + 1, n - 1, n + 1]
    assert total > sum(pieces)
    return pieces + [total - sum(pieces)]


# ---- a. pushes equal one shot, and the oracle ----

def test_pushes_equal_one_shot_and_the_float_oracle():
    plan = male_plan(precision=capi.PRECISION_F32)
    assert (plan.targets_filter_length(), one_row_chunk(capi.PRECISION_F32)) == (N, CHUNK)
    total = 3 * N + CHUNK + 5
    lists = cases.spoken_lists(total, 0, wide=True)
    want, want_maxabs = one_shot(plan, [lists], [total])
    stream = g.Stream(plan, 1)
    got, maxabs, _ = session(stream, [lists], lockstep_schedule(the_pieces(N, CHUNK, total), 1))
    same(got, maxabs, want, want_maxabs)
    assert got[0].size == plan.targets_output_count(total)
    # the float oracle at one step per frame on the host rule's frames
    frames, status = capi.targets_apply_host(plan, lists, total)
    assert status == 0
    rate = plan.info.internal_rate_hz
    cfg = oracle.male_config(44100.0, 1, float_model=1)
    assert oracle.derive(cfg, rate).control_steps == 1
    ref = oracle.synthesize(cfg, frames, control_rate=rate)
    assert ref.size == got[0].size and np.array_equal(got[0], ref)
    assert maxabs[0] == np.abs(got[0]).max()


def test_forty_pushes_of_one_step():
    plan = male_plan(precision=capi.PRECISION_F32)
    lists = cases.spoken_lists(40, 1, stride=5)
    want, want_maxabs = one_shot(plan, [lists], [40])
    got, maxabs, sizes = session(g.Stream(plan, 1), [lists], lockstep_schedule([1] * 40, 1))
    same(got, maxabs, want, want_maxabs)
    # every twelfth push launches, the rest only accumulate
    assert [size > 0 for size in sizes] == [(i + 1) % 12 == 0 for i in range(40)]


# ---- b. ragged batches: one utterance per workgroup ----

def test_ragged_batch_with_zeros_and_an_utterance_never_pushed():
    plan = male_plan(precision=capi.PRECISION_F32)
    schedule = [[13, 0, 145, 1, 0], [0, 7, 11, 300, 0], [N + 1, 5, 0, 0, 0], [12, 0, 24, 143, 0], [0, 0, 1, N - 1, 0], [144, 1, 0, 2, 0]]
    totals = [int(t) for t in np.sum(schedule, axis=0)]
    assert totals[4] == 0 and 0 in schedule[0][:4] and len(set(totals)) == 5
    utterances = [cases.spoken_lists(max(t, 1), 10 + b, wide=b == 3) for b, t in enumerate(totals)]
    want, want_maxabs = one_shot(plan, utterances, totals)
    got, maxabs, _ = session(g.Stream(plan, 5), utterances, schedule)
    same(got, maxabs, want, want_maxabs)


# ---- c. lockstep: utterances share workgroups ----

@pytest.mark.parametrize("kind,rows,delay,rate,n,chunk", [("rows2", 2, 1, 44100.0, 1002, 96), ("rows4", 4, 1, 44100.0, 1002, 48),
                                                        ("delay2-rows4", 4, 2, 44100.0, 2003, 48), ("down-16k", 4, 1, 16000.0, None, None)])
def test_lockstep_batches_in_forced_rows(kind, rows, delay, rate, n, chunk):
    plan = male_plan(precision=capi.PRECISION_F32, delay=delay, rate=rate, rows=rows)
    if n is None:
        n, chunk = plan.targets_filter_length(), int(plan._lib.gvtm_debug_chunk_length(plan._h, 5))
        assert plan.info.internal_rate_hz > rate
    assert (plan.targets_filter_length(), int(plan._lib.gvtm_debug_chunk_length(plan._h, 5))) == (n, chunk)
    pieces = [1, 11, 13, chunk + 1, n - 1, 2 * chunk + 12, n + 1, 7]
    total = sum(pieces)
    utterances = [cases.spoken_lists(total, 20 + b, wide=b == 1) for b in range(5)]
    want, want_maxabs = one_shot(plan, utterances, [total] * 5)
    got, maxabs, _ = session(g.Stream(plan, 5), utterances, lockstep_schedule(pieces, 5))
    same(got, maxabs, want, want_maxabs)


# ---- d. fp64 and mixed: the one-shot entry's bytes in that precision ----

@pytest.mark.parametrize("precision", [capi.PRECISION_F64, capi.PRECISION_MIXED], ids=["f64", "mixed"])
def test_double_classes_equal_their_one_shot(precision):
    plan = male_plan(precision=precision)
    n, chunk = plan.targets_filter_length(), one_row_chunk(precision)
    total = 3 * n + chunk + 5
    utterances = [cases.spoken_lists(total, 30 + b) for b in range(2)]
    want, want_maxabs = one_shot(plan, utterances, [total] * 2)
    got, maxabs, _ = session(g.Stream(plan, 2), utterances, lockstep_schedule(the_pieces(n, chunk, total), 2))
    same(got, maxabs, want, want_maxabs)


# ---- e. the log stays bounded ----

def test_the_log_stays_bounded_under_dense_points():
    plan = male_plan(precision=capi.PRECISION_F32)
    total = 3 * N + 18  # (a multiple of 24)
    assert total % 24 == 0
    lists = cases.spoken_lists(total, 40)
    for p in (0, 4, 9, 15):  # a point every 7 steps on four parameters, the list's own values in turn
        steps = list(range(0, total, 7))
        lists[p] = (steps, lists[p][1][np.arange(len(steps)) % len(lists[p][1])])
    want, want_maxabs = one_shot(plan, [lists], [total])
    stream = g.Stream(plan, 1)
    done, outs, held = 0, [], []
    while done < total:
        outs.append(stream.push_targets([sessions.slice_lists(lists, done, 24)], 24)[0])
        done += 24
        held.append(int(stream.targets_points()[0]))
    # the points of the last N + 12 steps, and one more per list
    bound = sum(1 for steps, _ in lists for s in steps if total - (N + 12) <= s < total) + 16
    assert held[-1] <= bound < sum(len(l[0]) for l in lists) // 2
    assert max(held) <= 4 * ((N + 12) // 7 + 1) + 12 * ((N + 12) // 211 + 1) + 16  # ... at any time of the session
    tail, maxabs = stream.finish()
    same([np.concatenate(outs + [tail[0]])], maxabs, want, want_maxabs)


# ---- f. a refused push leaves the stream as it was ----

def test_a_refused_push_changes_nothing():
    # (the stride of 8 samples is short: utterance 0 holds 101 steps then and synthesizes 96 of them)
    refused_push_changes_nothing(male_plan(precision=capi.PRECISION_F32), "push_targets", [400, 300, 300, 300, 350])


# ---- g. feeds and plans ----

def test_feeds_exclude_each_other_until_a_reset():
    plan = male_plan(precision=capi.PRECISION_F32)
    lists = cases.spoken_lists(200, 60)
    frames = np.zeros((1, 4, 16), np.float32)
    frames[:] = capi.targets_apply_host(plan, lists, 200)[0][199]
    stream = g.Stream(plan, 1)
    stream.push_targets([sessions.slice_lists(lists, 0, 30)], 30)
    with pytest.raises(g.GvtmError) as e:
        stream.push(frames)
    assert e.value.status == INVALID_ARGUMENT and "targets" in str(e.value)
    assert int(stream.targets_points()[0]) > 0
    stream.reset()
    assert int(stream.targets_points()[0]) == 0
    stream.push(frames)
    with pytest.raises(g.GvtmError) as e:
        stream.push_targets([sessions.slice_lists(lists, 0, 30)], 30)
    assert e.value.status == INVALID_ARGUMENT and "frames" in str(e.value)
    # after a reset a second session on the same object equals its own one shot
    stream.reset()
    want, want_maxabs = one_shot(plan, [lists], [200])
    got, maxabs, _ = session(stream, [lists], lockstep_schedule([30, 5, 150, 15], 1))
    same(got, maxabs, want, want_maxabs)
    # ... and a third, cut elsewhere, after a session that was not finished
    stream.reset()
    stream.push_targets([sessions.slice_lists(lists, 0, 77)], 77)
    stream.reset()
    got, maxabs, _ = session(stream, [lists], lockstep_schedule([1, 199], 1))
    same(got, maxabs, want, want_maxabs)


def test_unsupported_plans():
    offsets, steps, values = capi.pack_targets(cases.spoken_lists(10, 0) * 2)
    voices = g.VoicesPlan(configs(44100.0, 1, capi.PRECISION_F32, names=["male", "female"]), 250.0, 0)
    for stream in (g.Stream(voices, 2, voice_ids=[0, 1]), g.Stream(model5_plan("male"), 2)):
        stride = stream.targets_capacity(10)
        audio, counts = np.zeros((2, stride), np.float32), np.zeros(2, np.int64)
        rc = stream._lib.gvtm_stream_push_targets(stream._h, capi._ptr(offsets), capi._ptr(steps), capi._ptr(values), None, 10, capi._ptr(audio), stride,
                                                  capi._ptr(counts), None)
        assert rc == UNSUPPORTED
        assert stream.targets_points().tolist() == [0, 0]
