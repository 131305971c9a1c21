"""Streams fed parameter targets under a mix of voices, the models 0 to 4 (gvtm_stream_push_targets_voices on a stream of
gvtm_stream_create_voices; vtm_synth_kernel with the voices and the targets flag together on behalf of a stream).

The bar is the header's contract: for every voice v, the steps of an utterance of voice v pushed in any grouping and then
finished give, bit for bit and in every precision, the samples, count and maxabs of one gvtm_synthesize_targets_voices_device
call on the whole lists under voice v.  Every utterance walks its lists through its OWN voice's filter: the plans mix the
male and the female voice with the baby voice, which at 44.1 kHz down-samples (another ring, another state layout) and whose
filter is more than twice as long.  Sessions are cut by stream_targets_voices_cases with each voice's own N_v
(test_stream_targets_voices_cpu.py holds them to what they must cover); batches are ragged (one utterance per workgroup) and
in lockstep per voice (rows forced to 2 and 4).

No batch is above 13 utterances, no utterance longer than 3 N_v + chunk + 5 steps."""
import numpy as np
import pytest

import gama_tts_amd as g
from gama_tts_amd import capi
import oracle
import stream_targets_cases as sessions
import stream_targets_voices_cases as sv
import tracks
import voices_matrix_cases
from targets_cases import spoken_lists
from targets_io import one_shot as one_voice_one_shot, run_targets as one_shot_voices, same_as_one_shot, session
from voice_cases import configs, male_plan, model5_plan

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT, UNSUPPORTED = 1, 4
THREE = ["male", "female", "baby"]
IDS = (2, 0, 1, 0, 2)


def voices_plan(names, precision=capi.PRECISION_F32, rows=0):
    return g.VoicesPlan(configs(44100.0, 1, precision, names=names), 250.0, 0, diagnostics=bool(rows), rows=rows)


def one_row_chunk(precision):
    plan = male_plan(precision=precision, rows=1, device=capi.DEVICE_NONE)
    return int(plan._lib.gvtm_debug_chunk_length(plan._h, 1))


def filters(plan, count):
    return [plan.targets_filter_length(v) for v in range(count)]


def whole_session(plan, ids, utterances, pieces, stream=None):
    """The utterances pushed by their pieces on a stream of voices `ids` (a new one by default) and finished, against the
    one-shot voices entry on the whole lists -> the session's samples."""
    totals = [sum(p) for p in pieces]
    want = one_shot_voices(plan, utterances, totals, list(ids))
    assert not want[3].any()
    stream = stream or g.Stream(plan, len(ids), voice_ids=list(ids))
    got, maxabs, _ = session(stream, utterances, sv.schedule_of(pieces), push=stream.push_targets_voices)
    same_as_one_shot(got, maxabs, want, tuple(ids))
    for b, v in enumerate(ids):
        assert got[b].size == plan.targets_voice_output_count(v, totals[b]), b
    return got


# ---- a. equality with the one-shot voices entry ----

@pytest.mark.parametrize("precision", [capi.PRECISION_F32, capi.PRECISION_MIXED, capi.PRECISION_F64], ids=["f32", "mixed", "f64"])
def test_ragged_sessions_equal_the_one_shot_voices_entry(precision):
    plan = voices_plan(THREE, precision)
    n, chunk = filters(plan, 3), one_row_chunk(precision)
    assert len(set(n)) == 3 and n[2] > 2 * n[0]
    totals, pieces = sv.ragged_sessions(n, chunk, IDS)
    utterances = [spoken_lists(max(t, 1), 10 + b, wide=b == 2) for b, t in enumerate(totals)]
    got = whole_session(plan, IDS, utterances, pieces)
    assert got[3].size == plan.targets_voice_output_count(IDS[3], 0)  # (never pushed: the flush of nothing)
    if precision == capi.PRECISION_F32:
        # the male voice's utterance is also the float oracle's at one step per frame on the host rule's frames
        frames, status = capi.targets_apply_host(plan, utterances[1], totals[1], voice=0)
        assert status == 0 and IDS[1] == 0
        rate = male_plan(precision=precision, device=capi.DEVICE_NONE).info.internal_rate_hz
        cfg = oracle.male_config(44100.0, 1, float_model=1)
        assert oracle.derive(cfg, rate).control_steps == 1
        ref = oracle.synthesize(cfg, frames, control_rate=rate)
        assert ref.size == got[1].size and np.array_equal(got[1], ref)


@pytest.mark.parametrize("name,names,precision,rows,launched,chunk", sv.LOCKSTEP, ids=[c[0] for c in sv.LOCKSTEP])
def test_lockstep_per_voice_in_forced_rows(name, names, precision, rows, launched, chunk):
    plan = voices_plan(list(names), precision, rows=rows)
    ids = sv.LOCKSTEP_IDS[rows]
    # (what is launched, by the library's own hook: stream_targets_voices_cases.LOCKSTEP says why four float rows run as two)
    assert voices_matrix_cases.stream_launch_shape(plan, len(ids))[0] == launched
    totals, pieces = sv.lockstep_sessions(filters(plan, 3), chunk, ids)
    utterances = [spoken_lists(t, 20 + b, wide=b == 1) for b, t in enumerate(totals)]
    whole_session(plan, ids, utterances, pieces)


# ---- b. reset_voices: the next session runs under the new voices' filters ----

def test_sessions_after_reset_voices_equal_their_own_one_shot():
    plan = voices_plan(THREE)
    n = filters(plan, 3)
    stream = g.Stream(plan, 5, voice_ids=list(IDS))
    for round_, ids in enumerate((IDS, (0, 2, 2, 1, 0), (1, 1, 0, 2, 2))):
        if round_:
            stream.reset(voice_ids=list(ids))
        pieces = [[13, 25, n[v] - 7, 100 + 12 * b, 31] for b, v in enumerate(ids)]
        utterances = [spoken_lists(sum(p), 30 + 5 * round_ + b) for b, p in enumerate(pieces)]
        whole_session(plan, ids, utterances, pieces, stream)
        if round_ == 1:
            # ... and once more after a session that was not finished
            stream.reset(voice_ids=[2, 2, 2, 0, 0])
            stream.push_targets_voices([sessions.slice_lists(u, 0, 77) for u in utterances], 77)
            assert stream.targets_points().all()


# ---- c. the log's bound per voice, d. the capacity: voice 0's N once the largest, once the smallest ----

@pytest.mark.parametrize("names", [["baby", "male"], ["male", "baby"]], ids=["baby-first", "male-first"])
def test_the_log_is_bounded_by_each_utterances_own_window(names):
    plan = voices_plan(names)
    n = filters(plan, 2)
    total = (2 * max(n) + 240) // 120 * 120
    assert total > 2 * max(n) and max(n) > 2 * min(n)
    utterances = []
    for b in range(2):
        lists = spoken_lists(total, 40 + b)
        for p in (0, 4, 9, 15):  # a point every 7 steps on four parameters, the list's own values in turn
            steps = list(range(0, total, 7))
            lists[p] = (steps, lists[p][1][np.arange(len(steps)) % len(lists[p][1])])
        utterances.append(lists)
    stream = g.Stream(plan, 2, voice_ids=[0, 1])
    held = []

    def after_push(done):
        held.append(stream.targets_points().tolist())
        for b in range(2):
            assert held[-1][b] <= sv.log_bound(utterances[b], done[b], n[b]), (b, done)

    pieces = [[120] * (total // 120)] * 2
    want = one_shot_voices(plan, utterances, [total] * 2, [0, 1])
    got, maxabs, _ = session(stream, utterances, sv.schedule_of(pieces), after_push, push=stream.push_targets_voices)
    same_as_one_shot(got, maxabs, want, names)
    # (the shorter window holds fewer points: a log kept by the longer one would show here)
    short = n.index(min(n))
    assert held[-1][short] < held[-1][1 - short]


@pytest.mark.parametrize("names", [["baby", "male"], ["male", "baby"]], ids=["baby-first", "male-first"])
def test_capacity_is_the_largest_over_the_plans_voices(names):
    plan = voices_plan(names)
    S = 100
    lib, p = plan._lib, capi._ptr
    # (whichever voices the ids name: a stream of the male voice alone answers for the baby voice too)
    male_only = g.Stream(plan, 2, voice_ids=[names.index("male")] * 2)
    stream, twin = g.Stream(plan, 2, voice_ids=[0, 1]), g.Stream(plan, 2, voice_ids=[0, 1])
    cap = stream.targets_capacity(S)
    assert cap == male_only.targets_capacity(S) == plan.targets_voices_output_capacity(S + 11) + 1
    for v in range(2):
        assert cap >= plan.targets_voice_output_count(v, S + 11)
    utterances = [spoken_lists(3 * S, 60 + b) for b in range(2)]

    def raw_push(st, first, stride):
        offsets, steps, values = capi.pack_targets([l for u in utterances for l in sessions.slice_lists(u, first, S)])
        audio, counts, statuses = np.zeros((2, max(stride, 1)), np.float32), np.zeros(2, np.int64), np.full(2, -1, np.int32)
        rc = lib.gvtm_stream_push_targets_voices(st._h, p(offsets), p(steps), p(values), None, S, p(audio), stride, p(counts), p(statuses))
        return rc, audio, counts

    # a push of S steps with exactly that stride succeeds for both voices
    rc, audio, counts = raw_push(stream, 0, cap)
    assert rc == 0 and counts.min() > 0
    assert raw_push(twin, 0, cap)[0] == 0
    # the twin shows what the next push produces; a stride one short of it is refused and leaves the stream as found
    rc, want_audio, want_counts = raw_push(twin, S, cap)
    assert rc == 0
    need, held = int(want_counts.max()), stream.targets_points().tolist()
    rc, audio, counts = raw_push(stream, S, need - 1)
    assert rc == INVALID_ARGUMENT and b"audio_stride" in lib.gvtm_last_error() and not audio.any()
    assert stream.targets_points().tolist() == held
    rc, audio, counts = raw_push(stream, S, need)
    assert rc == 0 and counts.tolist() == want_counts.tolist()
    for b in range(2):
        assert audio[b, : counts[b]].tobytes() == want_audio[b, : counts[b]].tobytes(), b
    tails, peaks = stream.finish()
    twin_tails, twin_peaks = twin.finish()
    assert all(tails[b].tobytes() == twin_tails[b].tobytes() for b in range(2)) and peaks.tobytes() == twin_peaks.tobytes()


# ---- e. statuses and refusals ----

def test_statuses_and_refusals():
    plan = voices_plan(THREE)
    utterances = [spoken_lists(300, 70 + b) for b in range(3)]
    stream = g.Stream(plan, 3, voice_ids=[2, 0, 1])
    start = stream.push_targets_voices([sessions.slice_lists(u, 0, 13) for u in utterances], 13)
    held = stream.targets_points().tolist()
    # a bad list: the utterance's status, and nothing pushed
    bad = [sessions.slice_lists(u, 13, 100) for u in utterances]
    bad[1][3] = ([5], np.float32([np.nan]))
    bad[2][5] = ([0, 100], np.float32([1.0, 2.0]))
    with pytest.raises(g.GvtmError) as refused:
        stream.push_targets_voices(bad, 100)
    assert refused.value.status == INVALID_ARGUMENT and refused.value.statuses.tolist() == [0, 3, 4]
    assert stream.targets_points().tolist() == held
    # the corrected push and the rest of the session: the one shot's samples, nothing synthesized twice
    want = one_shot_voices(plan, utterances, [300] * 3, [2, 0, 1])
    first = stream.push_targets_voices([sessions.slice_lists(u, 13, 100) for u in utterances], 100)
    rest = stream.push_targets_voices([sessions.slice_lists(u, 113, 187) for u in utterances], 187)
    tail, maxabs = stream.finish()
    same_as_one_shot([np.concatenate([start[b], first[b], rest[b], tail[b]]) for b in range(3)], maxabs, want)
    with pytest.raises(g.GvtmError):
        stream.push_targets_voices(bad, 100)  # finished
    # a frames-fed stream is refused until a reset
    stream.reset()
    stream.push(tracks.random_tracks(3, 4, seed0=5, consonant_heavy=True))
    with pytest.raises(g.GvtmError) as e:
        stream.push_targets_voices([sessions.slice_lists(u, 0, 30) for u in utterances], 30)
    assert e.value.status == INVALID_ARGUMENT and "frames" in str(e.value)
    stream.reset()
    got, maxabs, _ = session(stream, utterances, [[150] * 3, [150] * 3], push=stream.push_targets_voices)
    same_as_one_shot(got, maxabs, want)
    # a model 5 stream has the other entry
    five = g.Stream(model5_plan("male"), 1)
    with pytest.raises(g.GvtmError) as e:
        five.push_targets_voices([sessions.slice_lists(utterances[0], 0, 10)], 10)
    assert e.value.status == UNSUPPORTED and "gvtm_stream_push_targets_model5_voices" in str(e.value)
    assert five.targets_points().tolist() == [0]


def test_on_a_one_voice_plan_the_old_and_the_new_entry_alternate():
    plan = male_plan(precision=capi.PRECISION_F32)
    total = plan.targets_filter_length() + 300
    lists = spoken_lists(total, 80)
    want, want_maxabs = one_voice_one_shot(plan, [lists], [total])
    stream = g.Stream(plan, 1)
    outs, done = [], 0
    for i, count in enumerate([13, 1, 144, 500, 7, total - 665]):
        push = stream.push_targets_voices if i % 2 == 0 else stream.push_targets
        outs.append(push([sessions.slice_lists(lists, done, count)], count)[0])
        done += count
    tail, maxabs = stream.finish()
    got = np.concatenate(outs + [tail[0]])
    assert got.tobytes() == want[0].tobytes() and maxabs.tobytes() == np.asarray(want_maxabs).tobytes()
