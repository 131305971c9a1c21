"""Streams that listen (gvtm_stream_listen, gvtm_stream_take_spectra, ...; csrc/vtm_listen.hip and the slot table of
csrc/vtm_analysis.hip): the interactive window's analysis ring on the device, for every utterance of a stream.

The bar is the header's contract, and it is equality of bits: utterance b's queued spectra and signal views, fed in any
grouping by any feed, are the rows of what gvtm_analyze_spectrum_device writes, for the same analysis object and first = 0, on
the utterance's whole sample sequence -- the one-shot entry's row where the stream contract makes the samples the same (a.),
the session's own downloaded, concatenated samples for the other feeds and families (b.).  The arithmetic of the analysis does
not depend on where a buffer lies; only the width of its loads does.

The ring is 65 536 output samples, about 1.5 s of audio, so every session is that long at least; batches are 1 to 3."""
import functools

import numpy as np
import pytest

import analysis_cases as ac
import gama_tts_amd as g
from gama_tts_amd import capi
import stream_targets_cases as sessions
import targets_cases
from targets_io import one_shot
import tracks
from test_gpu_analysis import check_against_host, run_device
from test_gpu_events_chunks import audio_plan
from test_gpu_stream_events import stream_utterances
from voice_cases import configs, male_plan, model5_plan

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT, NO_DEVICE = 1, 2
N = ac.N
CONFIGS = {"blackman-log": (ac.BLACKMAN, 65536, True, -120.0, 0.0), "rectangular-linear-cut": (ac.RECTANGULAR, 1024, False, -120.0, 5000.0)}


def analysis(name, rate=44100, device=0):
    kind, W, log_scale, min_db, max_freq = CONFIGS[name]
    return g.Analysis(kind, W, log_scale, min_db, max_freq, rate, device=device)


def steps_for(plan, samples):
    """The fewest steps of a targets-fed utterance that finishes with at least `samples` samples."""
    lo, hi = 1, 400000
    while lo < hi:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if plan.targets_output_count(mid) >= samples else (mid + 1, hi)
    return lo


class Heard:
    """What the takes of a session returned, utterance by utterance in order.  Every take checks that the host rows behind an
    utterance's count kept their fill and that the queues are empty afterwards."""

    def __init__(self, stream):
        self.stream = stream
        self.spectra, self.signal = [[] for _ in range(stream.batch)], [[] for _ in range(stream.batch)]
        self.taken = []

    def take(self):
        spec, sig, n = self.stream.take_spectra(fill=np.nan)
        for b in range(self.stream.batch):
            for rows, kept in ((spec, self.spectra), (sig, self.signal)):
                if rows is not None:
                    assert np.isnan(rows[b, n[b]:]).all(), b  # the sentinel
                    kept[b] += [rows[b, k].copy() for k in range(n[b])]
        self.taken.append(n.copy())
        assert not self.stream.listen_state()[1].any()
        return n

    def counts(self):
        return np.sum(self.taken, axis=0)


def same_views(heard, want_spectra, want_signal, want_buffers):
    """The session's views against the analysis entry's rows, byte for byte, and the counts."""
    assert heard.counts().tolist() == want_buffers.tolist()
    for b, n in enumerate(want_buffers):
        for got, want in ((heard.spectra[b], want_spectra), (heard.signal[b], want_signal)):
            if want is not None:
                assert len(got) == n, b
                for k in range(n):
                    assert got[k].tobytes() == want[b, k].tobytes(), (b, k)


def as_arrays(heard, max_buffers, n_bins, W):
    """The session's views in the analysis entry's layout, NaN behind an utterance's buffers."""
    batch = heard.stream.batch
    spectra, signal = np.full((batch, max_buffers, n_bins), np.nan, np.float32), np.full((batch, max_buffers, W), np.nan, np.float32)
    for b in range(batch):
        for k, row in enumerate(heard.spectra[b]):
            spectra[b, k] = row
        for k, row in enumerate(heard.signal[b]):
            signal[b, k] = row
    return spectra, signal, heard.counts().astype(np.int32)


def targets_session(stream, utterances, schedule, heard=None, audio=True, entry="push_targets", after_push=None):
    """Pushes schedule[i][b] steps of utterance b in push i, then finishes; with `heard`, a take after every call -> (samples per
    utterance, or without audio their total counts; per call the samples each utterance received)."""
    batch = len(utterances)
    done, outs, sizes = [0] * batch, [[] for _ in range(batch)], []
    for i, counts in enumerate(schedule):
        given = [sessions.slice_lists(utterances[b], done[b], int(counts[b])) for b in range(batch)]
        got = getattr(stream, entry)(given, np.asarray(counts, dtype=np.int32), audio=audio)
        for b in range(batch):
            outs[b].append(got[b])
            done[b] += int(counts[b])
        sizes.append([int(got[b].size if audio else got[b]) for b in range(batch)])
        if after_push:
            after_push(i)
        if heard:
            heard.take()
    tail, _ = stream.finish(audio=audio)
    sizes.append([int(tail[b].size if audio else tail[b]) for b in range(batch)])
    if heard:
        heard.take()
    if not audio:
        return [sum(s[b] for s in sizes) for b in range(batch)], sizes
    return [np.concatenate(outs[b] + [tail[b]]) for b in range(batch)], sizes


# ---- a. sessions equal one shot ----

@functools.lru_cache(maxsize=None)
def trio():
    """Three ragged utterances of the float male plan: two buffers and a remainder, one buffer by the smallest margin the
    steps allow, none (one step fewer) -> (plan, lists, step totals, the push of more than 2 x 65536 samples, the one-shot
    entry's rows).  Computed once, shared, left unchanged."""
    plan = male_plan(precision=capi.PRECISION_F32)
    one = steps_for(plan, N)
    # (a push may keep up to 11 steps back, and the count steps_for measures includes the samples only a finish flushes)
    big = steps_for(plan, 2 * N) + 120
    totals = [13 + 24 + 11 + big + 40, one, one - 1]
    assert 2 * N < plan.targets_output_count(totals[0]) < 3 * N
    assert plan.targets_output_count(totals[2]) < N <= plan.targets_output_count(totals[1])
    utterances = [targets_cases.spoken_lists(t, 70 + b) for b, t in enumerate(totals)]
    rows, _ = one_shot(plan, utterances, totals)
    return plan, utterances, totals, big, rows


def trio_schedule():
    _, _, totals, big, _ = trio()
    half = (totals[1] - 36) // 2
    schedule = [[13, 25, 0], [24, 11, 7], [11, 0, 12], [big, half, totals[2] - 19], [40, totals[1] - 36 - half, 0]]
    assert [sum(col) for col in zip(*schedule)] == totals
    return schedule


@functools.lru_cache(maxsize=None)
def trio_reference(name):
    """gvtm_analyze_spectrum_device on the one-shot entry's rows."""
    return run_device(analysis(name), trio()[4], None, 2)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_sessions_equal_one_shot(name):
    plan, utterances, totals, big, rows = trio()
    want_spectra, want_signal, want_buffers = trio_reference(name)
    assert want_buffers.tolist() == [2, 1, 0]
    an = analysis(name)
    stream = g.Stream(plan, 3)
    stream.listen(an, 2, spectra=True, signal=True)
    heard, fills = Heard(stream), []
    got, sizes = targets_session(stream, utterances, trio_schedule(), heard, after_push=lambda i: fills.append(stream.listen_state()))
    for b in range(3):
        assert got[b].tobytes() == rows[b].tobytes(), b  # (the stream contract: what makes the one-shot rows the reference)
    same_views(heard, want_spectra, want_signal, want_buffers)
    # what the schedule is there for: odd and even fills, a push of 0 steps, one push of more than 2 x 65536 samples that
    # completes the ring it straddles and a buffer inside itself, and a ring that stays incomplete at the finish
    small = [int(f) for fill, _ in fills[:3] for f in fill if f]
    assert any(f % 2 for f in small) and any(f % 2 == 0 for f in small), small
    assert sizes[2][1] == 0 and sizes[3][0] > 2 * N
    assert fills[3][1].tolist()[0] == 2 and heard.taken[3][0] == 2
    fill, queued = stream.listen_state()
    assert fill.tolist() == [r.size % N for r in rows] and fill[2] == rows[2].size and not queued.any()
    assert [sum(s[b] for s in sizes) for b in range(3)] == [r.size for r in rows]
    if not CONFIGS[name][2]:
        # the linear spectra also meet the analysis entry's own bars against the host entry
        host = analysis(name, device=capi.DEVICE_NONE)
        spectra, signal, buffers = as_arrays(heard, 2, an.n_bins, an.window_size)
        check_against_host(host, host.window(), rows, None, 2, spectra, signal, buffers, label="listening " + name)


# ---- b. every feed and family ----

def frames_session(stream, params, pieces, heard):
    """params [batch][F][16] pushed in lockstep pieces, then finished, a take after every call -> samples per utterance."""
    outs, at = [[] for _ in range(stream.batch)], 0
    for n in pieces:
        for b, piece in enumerate(stream.push(params[:, at: at + n])):
            outs[b].append(piece)
        at += n
        heard.take()
    assert at == params.shape[1]
    tails, _ = stream.finish()
    heard.take()
    return [np.concatenate(outs[b] + [tails[b]]) for b in range(stream.batch)]


def events_session(stream, utterances, heard):
    """One chunk per utterance and push, then finished."""
    outs = [[] for _ in utterances]
    for k in range(max(len(u) for u in utterances)):
        got, _ = stream.push_events([u[k: k + 1] for u in utterances])
        for b, piece in enumerate(got):
            outs[b].append(piece)
        heard.take()
    tails, _ = stream.finish()
    heard.take()
    return [np.concatenate(outs[b] + [tails[b]]) for b in range(len(utterances))]


@pytest.mark.parametrize("family", ["two-voices-frames", "events", "model5-float-targets", "f64-frames"])
def test_every_feed_and_family(family):
    rate = 44100
    if family == "two-voices-frames":
        plan = g.VoicesPlan(configs(44100.0, 1, capi.PRECISION_F32, names=["male", "female"]), 250.0, 0)
        stream = g.Stream(plan, 2, voice_ids=[0, 1])
        params = np.stack([tracks.random_track(400, 80 + b) for b in range(2)]).astype(np.float32)
        run = lambda heard: frames_session(stream, params, [100, 151, 149], heard)  # noqa: E731
    elif family == "events":
        plan = audio_plan("f32")
        stream = g.Stream(plan, 2, voice_ids=[0, 0])
        run = lambda heard: events_session(stream, stream_utterances()[:2], heard)  # noqa: E731
    elif family == "model5-float-targets":
        rate = 48000
        plan = model5_plan("male", float_class=True)
        total = steps_for(plan, N) + 2001
        lists = targets_cases.spoken_lists(total, 90)
        schedule = [[1001], [4003], [total - 5004]]
        run = lambda heard: targets_session(stream, [lists], schedule, heard, entry="push_targets_model5")[0]  # noqa: E731
        stream = g.Stream(plan, 1)
    else:
        plan = male_plan(precision=capi.PRECISION_F64)
        stream = g.Stream(plan, 1)
        params = tracks.random_track(400, 95).astype(np.float32)[None]
        run = lambda heard: frames_session(stream, params, [7, 250, 143], heard)  # noqa: E731
    an = analysis("blackman-log", rate)
    stream.listen(an, 1, spectra=True, signal=True)
    heard = Heard(stream)
    rows = run(heard)
    assert all(N < r.size < 2 * N for r in rows), [r.size for r in rows]  # one buffer and a remainder
    want_spectra, want_signal, want_buffers = run_device(an, rows, None, 1)
    assert want_buffers.tolist() == [1] * len(rows)
    same_views(heard, want_spectra, want_signal, want_buffers)
    assert stream.listen_state()[0].tolist() == [r.size - N for r in rows]


# ---- c. audio is optional ----

def test_audio_is_optional_on_a_listening_stream_only():
    plan, utterances, totals, _, rows = trio()
    want_spectra, want_signal, want_buffers = trio_reference("blackman-log")
    streams = [g.Stream(plan, 3) for _ in range(2)]
    an = analysis("blackman-log")
    results = []
    for stream, audio in zip(streams, (True, False)):
        stream.listen(an, 2, spectra=True, signal=True)
        heard = Heard(stream)
        got, sizes = targets_session(stream, utterances, trio_schedule(), heard, audio=audio)
        same_views(heard, want_spectra, want_signal, want_buffers)
        results.append((got, sizes, stream.listen_state()[0].tolist()))
    assert results[1][0] == [r.size for r in rows] == [a.size for a in results[0][0]]
    assert results[1][1] == results[0][1] and results[1][2] == results[0][2]  # out_counts call by call, and the rings' fills
    # a stream that does not listen refuses a null audio with samples due, as ever
    plain = g.Stream(plan, 3)
    given = [sessions.slice_lists(utterances[b], 0, n) for b, n in enumerate(trio_schedule()[0])]
    with pytest.raises(g.GvtmError) as refused:
        plain.push_targets(given, np.asarray(trio_schedule()[0], dtype=np.int32), audio=False)
    assert refused.value.status == INVALID_ARGUMENT and "null audio" in str(refused.value)
    assert not plain.targets_points().any()
    with pytest.raises(g.GvtmError) as refused:
        plain.listen_state()
    assert refused.value.status == INVALID_ARGUMENT


# ---- d. the queue ----

def device_array(address, shape, dtype):
    """A device address as a tensor (no copy)."""
    import torch

    class Raw:
        pass

    raw = Raw()
    raw.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": np.dtype(dtype).str, "data": (int(address), False), "version": 2}
    return torch.as_tensor(raw, device="cuda:0")


def test_a_full_queue_refuses_the_push_until_a_take():
    plan, utterances, totals, _, _ = trio()
    want_spectra, want_signal, want_buffers = trio_reference("blackman-log")
    an = analysis("blackman-log")
    stream = g.Stream(plan, 3)
    stream.listen(an, 1, spectra=True, signal=True)
    heard = Heard(stream)
    piece, done, refused_at, calls = 14000, [0, 0, 0], [], 0
    assert 2 * plan.targets_output_count(piece) < N  # no push completes two rings
    while any(d < t for d, t in zip(done, totals)):
        counts = [min(piece, t - d) for d, t in zip(done, totals)]
        given = [sessions.slice_lists(utterances[b], done[b], counts[b]) for b in range(3)]
        push = lambda: stream.push_targets(given, np.asarray(counts, dtype=np.int32), audio=False)  # noqa: E731
        before = [a.tolist() for a in stream.listen_state()] + [stream.targets_points().tolist()]
        try:
            push()
        except g.GvtmError as refusal:
            # a second completed buffer for utterance 0 and no room: refused, and the stream exactly as found
            assert refusal.status == INVALID_ARGUMENT and "utterance 0" in str(refusal) and before[1][0] == 1
            assert [a.tolist() for a in stream.listen_state()] + [stream.targets_points().tolist()] == before
            refused_at.append(calls)
            # what the device queues show is what the take then returns
            d_spectra, d_signal, d_queued = stream.peek_spectra_device()
            peeked = [device_array(d_spectra, (3, 1, an.n_bins), np.float32).cpu().numpy(), device_array(d_signal, (3, 1, N), np.float32).cpu().numpy(),
                      device_array(d_queued, (3,), np.int32).cpu().numpy()]
            assert peeked[2].tolist() == before[1]
            n = heard.take()
            assert n.tolist() == before[1]
            for b in range(3):
                if n[b]:
                    assert peeked[0][b, 0].tobytes() == heard.spectra[b][-1].tobytes() and peeked[1][b, 0].tobytes() == heard.signal[b][-1].tobytes()
            push()  # the same push, after the take
        calls += 1
        done = [d + c for d, c in zip(done, counts)]
    stream.finish(audio=False)
    heard.take()
    assert len(refused_at) == 1
    same_views(heard, want_spectra, want_signal, want_buffers)  # (test a's reference)
    # a view the listener does not keep
    spectra_only = g.Stream(plan, 1)
    spectra_only.listen(an, 1, spectra=True, signal=False)
    signal = np.zeros((1, 1, N), np.float32)
    assert spectra_only._lib.gvtm_stream_take_spectra(spectra_only._h, None, capi._ptr(signal), None) == INVALID_ARGUMENT
    assert spectra_only.peek_spectra_device()[1] is None


# ---- e. life cycle ----

def test_life_cycle():
    plan = male_plan(precision=capi.PRECISION_F32)
    total = steps_for(plan, N) + 500
    lists = targets_cases.spoken_lists(total, 99)
    schedule = [[5000], [12001], [total - 17001]]
    an = analysis("rectangular-linear-cut")
    stream = g.Stream(plan, 1)
    # refusals: a mismatched sample rate, a design-only object, bad arguments, a stream already fed
    for bad, status in ((analysis("rectangular-linear-cut", rate=48000), INVALID_ARGUMENT), (analysis("rectangular-linear-cut", device=capi.DEVICE_NONE), NO_DEVICE)):
        with pytest.raises(g.GvtmError) as refused:
            stream.listen(bad, 1)
        assert refused.value.status == status
    for max_buffers, views in ((0, 1), (1, 0), (1, 4)):
        assert stream._lib.gvtm_stream_listen(stream._h, an._h, max_buffers, views) == INVALID_ARGUMENT
    stream.push_targets([sessions.slice_lists(lists, 0, 24)], 24)
    with pytest.raises(g.GvtmError) as refused:
        stream.listen(an, 1)
    assert refused.value.status == INVALID_ARGUMENT and "fed" in str(refused.value)
    with pytest.raises(g.GvtmError):
        stream.listen_state()
    stream.reset()
    stream.listen(an, 2, spectra=True, signal=True)
    stream.listen(an, 1, spectra=True, signal=True)  # (a fresh stream: the listener is replaced)
    first = Heard(stream)
    samples, _ = targets_session(stream, [lists], schedule, first)
    assert first.counts().tolist() == [1] and stream.listen_state()[0].tolist() == [samples[0].size - N]
    # a reset empties the ring, and the queue of a session that was not taken from
    stream.reset()
    assert [a.tolist() for a in stream.listen_state()] == [[0], [0]]
    targets_session(stream, [lists], schedule)
    assert [a.tolist() for a in stream.listen_state()] == [[samples[0].size - N], [1]]
    stream.reset()
    assert [a.tolist() for a in stream.listen_state()] == [[0], [0]]
    # a second session through the same listener reproduces the first
    second = Heard(stream)
    again, _ = targets_session(stream, [lists], schedule, second)
    assert again[0].tobytes() == samples[0].tobytes()
    assert [t.tolist() for t in second.taken] == [t.tolist() for t in first.taken]
    assert second.spectra[0][0].tobytes() == first.spectra[0][0].tobytes() and second.signal[0][0].tobytes() == first.signal[0][0].tobytes()
    # after unlisten the stream is one that never listened
    stream.reset()
    stream.push_targets([sessions.slice_lists(lists, 0, 24)], 24)
    stream.unlisten()  # (allowed at any time)
    with pytest.raises(g.GvtmError):
        stream.listen_state()
    stream.reset()
    plain, _ = targets_session(stream, [lists], schedule)
    never, _ = targets_session(g.Stream(plan, 1), [lists], schedule)
    assert plain[0].tobytes() == never[0].tobytes() == samples[0].tobytes()
