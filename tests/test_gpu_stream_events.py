"""Streams fed event lists (gvtm_stream_push_events; vtm_tracks_kernel<TrackAppendArgs>, vtm_carry_rows_kernel).

A stream that receives its utterances chunk by chunk, as the reference's Controller produces them, generates the frames on
the device behind the frames it still holds, synthesizes what can be synthesized and moves the rest to the front of its
frame buffer.  The two kernels are checked alone on buffers surrounded by sentinels (the diagnostics library's hooks); the
stream is checked against the one-shot entry on the whole utterances (gvtm_synthesize_events_chunks_device: samples,
counts, peaks, frame counts and drift states, bit for bit, however the chunks are grouped into pushes), against the float
oracle, and push by push against a frames-fed stream given the chained tracks oracle's frames."""
import functools
import math

import numpy as np
import pytest

from gama_tts_amd import capi
import oracle
import tracks
from chunk_cases import DIVERSE_TRACKS, GUARD_FRAMES, SENTINEL, chain_oracle, chunks_on_device, list_with_frames, synthesize_chunks
from device_io import to_device, to_host
from test_gpu_events_chunks import AUDIO_TRACKS, BAD_VOICE, ORACLE_TRACK, audio_plan, edge_batch, frame_count
from track_cases import fresh_drift, make_singable, product_config, singable_event_table, used_drift
from voice_cases import configs, male_plan

import gama_tts_amd as g

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT = 1


def sentinel_rows(rows):
    """rows x 16 floats of SENTINEL on the device, as int32 (the kernels see them as float32)."""
    import torch
    return torch.full((rows * 16,), SENTINEL, dtype=torch.int32, device="cuda:0")


# ---- 1. the append kernel alone

ROW_STARTS = (0, 1, 5, 12, 31, 32)


def test_append_kernel_writes_behind_the_held_rows_and_inside_the_block():
    utterances, ids = edge_batch()
    batch = len(utterances)
    assert batch == 11
    row_start = np.array([ROW_STARTS[(b + 2) % 6] for b in range(batch)], dtype=np.int32)
    assert set(row_start) == set(ROW_STARTS)
    drift0 = used_drift(batch)
    want = [chain_oracle(DIVERSE_TRACKS[v], u, drift0[b]) if v != BAD_VOICE else None for b, (u, v) in enumerate(zip(utterances, ids))]
    ends = sorted((int(row_start[b]) + w[0].shape[0], b) for b, w in enumerate(want) if w)
    # the rows: every utterance but the longest fits, and the longest is cut inside one of its chunks
    cap = ends[-2][0] + 3
    cut_b = ends[-1][1]
    room = cap - int(row_start[cut_b])
    boundaries = np.cumsum([frame_count(DIVERSE_TRACKS[ids[cut_b]], [t]) for t in utterances[cut_b]])
    assert 0 < room < want[cut_b][0].shape[0] and room not in boundaries
    assert all(int(row_start[b]) < cap for b in range(batch))

    plan = g.VoicesPlan(configs(precision=capi.PRECISION_F32), 250.0, 0, diagnostics=True)
    plan.set_voice_tracks([product_config(c) for c in DIVERSE_TRACKS])
    d_events, d_chunk_offsets, d_utt_chunks = chunks_on_device(utterances)
    d_ids, d_start, d_drift = to_device(np.asarray(ids, dtype=np.int32), row_start, np.ascontiguousarray(drift0, dtype=np.float64).copy())
    buf = sentinel_rows(batch * cap + GUARD_FRAMES)
    d_counts, = to_device(np.full(batch, 99, dtype=np.int32))
    rc = plan._lib.gvtm_debug_tracks_append(plan._h, capi._ptr(d_events), capi._ptr(d_chunk_offsets), capi._ptr(d_utt_chunks), capi._ptr(d_ids),
                                            capi._ptr(d_start), batch, cap, capi._ptr(buf), capi._ptr(d_counts), capi._ptr(d_drift))
    assert rc == 0, plan._lib.gvtm_last_error()
    out, counts, drift = to_host(buf, d_counts, d_drift)
    out = out.view(np.uint32)
    assert (out[batch * cap * 16:] == SENTINEL).all(), "written past the last block"
    blocks = out[: batch * cap * 16].reshape(batch, cap, 16)
    for b, w in enumerate(want):
        if w is None:
            assert counts[b] == 0 and (blocks[b] == SENTINEL).all(), b
            assert drift[b].tobytes() == np.asarray(drift0[b], dtype=np.float64).tobytes(), b
            continue
        frames, state = w
        lo = int(row_start[b])
        n = min(frames.shape[0], cap - lo)
        assert counts[b] == frames.shape[0], (b, int(counts[b]), frames.shape[0])
        assert (blocks[b, :lo] == SENTINEL).all(), b
        assert np.array_equal(blocks[b, lo: lo + n], frames[:n].view(np.uint32)), b
        assert (blocks[b, lo + n:] == SENTINEL).all(), b
        assert drift[b].tobytes() == np.array(state, dtype=np.float64).tobytes(), b
    assert counts[cut_b] > cap - row_start[cut_b] and counts[0] == 0


# ---- 2. the carry kernel alone

def test_carry_kernel_moves_the_kept_rows_to_the_front():
    cases = [(n, kept) for n in (0, 12, 24) for kept in (1, 2, 11, 12)]
    cases += [(5, 12), (1, 16)]  # rows that move onto themselves; as many rows as the kernel moves
    done, held = [], []
    for n, kept in cases:  # every case between two blocks in which nothing is held
        done += [0, n]
        held += [0, n + kept]
    done, held = np.array(done + [0], dtype=np.int32), np.array(held + [0], dtype=np.int32)
    batch, cap = done.shape[0], 40
    assert batch % 2 == 1 and held.max() < cap
    rng = np.random.default_rng(7)
    before = np.full((batch + 2, cap, 16), SENTINEL, dtype=np.uint32)  # (a guard of one block on either side)
    for b in range(batch):
        before[1 + b, done[b]: held[b]] = rng.integers(0, 1 << 30, (held[b] - done[b], 16), dtype=np.uint32)
    want = before.copy()
    for b in range(batch):
        want[1 + b, : held[b] - done[b]] = before[1 + b, done[b]: held[b]]
    buf, d_done, d_held = to_device(before.view(np.int32), done, held)
    plan = male_plan(diagnostics=True)
    rc = plan._lib.gvtm_debug_carry_rows(plan._h, buf.data_ptr() + cap * 64, capi._ptr(d_done), capi._ptr(d_held), batch, cap)
    assert rc == 0, plan._lib.gvtm_last_error()
    got, = to_host(buf)
    got = got.view(np.uint32)
    for b in range(batch):
        assert np.array_equal(got[1 + b], want[1 + b]), (b, int(done[b]), int(held[b]))
    assert (got[0] == SENTINEL).all() and (got[-1] == SENTINEL).all()


# ---- 3. the stream against the one-shot entry

KINDS = ["f32", "f64", "model5_f32"]
SINGABLE = [(300, 40), (301, 2), (302, 1), (303, 17), (305, 3), (306, 55), (307, 9), (308, 33), (309, 25)]
IDS = [0, 0, 1, 2, 3, 4, 0, 1, 2]


@functools.lru_cache(maxsize=None)
def stream_utterances():
    """Nine utterances of 0 to 4 chunks: rows 0 and 1 the two oracle utterances (voice 0); utterance 4 has a chunk of one
    frame in the middle."""
    S = {sn: singable_event_table(*sn) for sn in SINGABLE}
    f1 = make_singable(list_with_frames(1))
    return [[S[300, 40], S[303, 17], S[306, 55]],
            [S[308, 33], S[309, 25], S[300, 40], S[303, 17]],
            [S[306, 55]], [], [S[301, 2], f1, S[307, 9]], [S[302, 1], S[305, 3], S[303, 17]], [S[309, 25], S[308, 33]],
            [S[300, 40]], [S[307, 9], S[302, 1], S[305, 3]]]


def schedule(name):
    """-> the pushes: per push and utterance, how many of the utterance's next chunks it brings."""
    sizes = [len(u) for u in stream_utterances()]
    if name == "one_chunk_per_push":
        return [[1 if k < n else 0 for n in sizes] for k in range(max(sizes))]
    if name == "all_at_once":
        return [sizes]
    # ragged: a small first push (two utterances, five frames), then one many times larger while utterance 4 holds
    # rows; a push that brings nothing but the one-frame chunk; the utterances advance in different pushes
    pushes = [[0, 0, 0, 0, 1, 1, 0, 0, 0],
              [2, 2, 1, 0, 0, 0, 0, 0, 0],
              [0, 0, 0, 0, 1, 0, 0, 0, 0],
              [1, 2, 0, 0, 1, 2, 1, 1, 3],
              [0, 0, 0, 0, 0, 0, 1, 0, 0]]
    assert [sum(col) for col in zip(*pushes)] == sizes
    return pushes


SCHEDULES = ["one_chunk_per_push", "all_at_once", "ragged"]


def pushes_of(name):
    """-> per push: utterance b's chunks of that push (lists of event tables)."""
    utterances = stream_utterances()
    at = [0] * len(utterances)
    out = []
    for take in schedule(name):
        out.append([u[at[b]: at[b] + take[b]] for b, u in enumerate(utterances)])
        at = [a + t for a, t in zip(at, take)]
    return out


def drift0():
    return used_drift(len(IDS))


@functools.lru_cache(maxsize=None)
def one_shot(kind):
    """gvtm_synthesize_events_chunks_device on the whole utterances: computed once per kind, shared, left unchanged."""
    utterances = stream_utterances()
    frames_of = [frame_count(AUDIO_TRACKS[v], u) for u, v in zip(utterances, IDS)]
    assert frames_of[:2] == [673, 702] and frames_of[3] == 0 and max(frames_of) == 702
    plan = audio_plan(kind)
    out = synthesize_chunks(plan, utterances, IDS, max(frames_of), plan.voices_output_capacity(max(frames_of)), drift0(), entry=True)
    assert out["frames"].tolist() == frames_of
    return out


def granules(plan):
    """Frames per voice in whose multiples a push synthesizes (include/gama_vtm.h, "Streams": 12 internal steps; model 5: 4)."""
    block = 4 if plan.info.model5 else 12
    return [block // math.gcd(plan.voice_info(v).control_steps, block) for v in range(plan.n_voices)]


def run_events_stream(plan, pushes, strides=None):
    """The pushes through a fresh events-fed stream that starts from drift0() -> (per push: samples per utterance; per push:
    frames generated; rows held when each push began; tails, maxabs, final drift states)."""
    st = g.Stream(plan, len(IDS), voice_ids=IDS)
    st.set_drift(drift0())
    gran = granules(plan)
    held = np.zeros(len(IDS), dtype=np.int64)
    samples, frames, held_at = [], [], []
    for p, push in enumerate(pushes):
        held_at.append(held.copy())
        got, new = st.push_events(push, None if strides is None else strides[p])
        samples.append(got)
        frames.append(new)
        have = held + new
        held = np.array([h - ((h - 1) // gran[v]) * gran[v] if h > 0 else 0 for h, v in zip(have, IDS)])
    tails, maxabs = st.finish()
    return samples, frames, held_at, tails, maxabs, st.get_drift()


@pytest.mark.parametrize("name", SCHEDULES)
@pytest.mark.parametrize("kind", KINDS)
def test_events_fed_stream_equals_the_one_shot_entry(kind, name):
    ref = one_shot(kind)
    utterances = stream_utterances()
    samples, frames, held_at, tails, maxabs, drift = run_events_stream(audio_plan(kind), pushes_of(name))
    for b in range(len(IDS)):
        whole = np.concatenate([s[b] for s in samples] + [tails[b]])
        assert whole.size == ref["counts"][b], (b, whole.size, int(ref["counts"][b]))
        assert whole.tobytes() == ref["audio"][b, : whole.size].tobytes(), b
        assert sum(int(f[b]) for f in frames) == ref["frames"][b], b
    assert maxabs.tobytes() == ref["maxabs"].tobytes()
    assert drift.tobytes() == ref["drift"].tobytes()
    # the empty utterance: no frames, and the samples the one-shot entry gives it
    assert all(f[3] == 0 for f in frames) and tails[3].size == ref["counts"][3]
    if name == "ragged":
        # a push that returned no samples for an utterance that held frames, and one that began with two rows or more held
        assert any(held_at[p][b] > 0 and samples[p][b].size == 0 for p in range(len(samples)) for b in range(len(IDS)))
        assert max(h.max() for h in held_at) >= 2
        # the frame buffer grows while rows are held: the second push is at least eight times the first
        assert held_at[1].max() > 0 and frames[1].max() >= 8 * (frames[0].max() + 1)
        # the push of the one-frame chunk alone
        assert frames[2].tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 0]
    if kind != "f32":
        return
    # bit identity is the float path's contract: the float oracle on the chained tracks oracle's frames
    for b in (0, 1):
        chained, state = chain_oracle(ORACLE_TRACK, utterances[b], drift0()[b])
        want = oracle_audio(b)
        whole = np.concatenate([s[b] for s in samples] + [tails[b]])
        assert chained.shape[0] == ref["frames"][b] and whole.size == want.size
        assert whole.tobytes() == want.tobytes(), b
        assert drift[b].tobytes() == np.array(state, dtype=np.float64).tobytes()


@functools.lru_cache(maxsize=None)
def oracle_audio(b):
    """The float oracle's samples of utterance b (0 or 1, voice 0) on the chained tracks oracle's frames."""
    chained, _ = chain_oracle(ORACLE_TRACK, stream_utterances()[b], drift0()[b])
    ref = oracle.synthesize(oracle.male_config(44100.0, 1, float_model=1), chained)
    assert np.isfinite(ref).all()
    return ref


# ---- 4. push by push against a frames-fed stream

@pytest.mark.parametrize("kind", KINDS)
def test_every_push_equals_the_frames_fed_stream(kind):
    plan = audio_plan(kind)
    pushes = pushes_of("ragged")
    samples, frames, _, tails, maxabs, _ = run_events_stream(plan, pushes)
    st = g.Stream(plan, len(IDS), voice_ids=IDS)
    state = [tuple(d) for d in drift0()]
    for p, push in enumerate(pushes):
        rows = []
        for b, chunks in enumerate(push):  # the chained oracle's frames of this push's chunks, the state handed on
            part, state[b] = chain_oracle(AUDIO_TRACKS[IDS[b]], chunks, state[b])
            rows.append(part)
        counts = np.array([r.shape[0] for r in rows], dtype=np.int32)
        assert counts.tolist() == frames[p].tolist()
        buf = np.zeros((len(IDS), max(1, int(counts.max())), 16), dtype=np.float32)
        for b, r in enumerate(rows):
            buf[b, : r.shape[0]] = r
        got = st.push(buf, counts)
        for b in range(len(IDS)):
            assert got[b].size == samples[p][b].size and got[b].tobytes() == samples[p][b].tobytes(), (p, b)
    f_tails, f_maxabs = st.finish()
    for b in range(len(IDS)):
        assert f_tails[b].tobytes() == tails[b].tobytes(), b
    assert f_maxabs.tobytes() == maxabs.tobytes()


# ---- 5. feeding modes, refusals, the drift generators across resets

def status_of(call, *args):
    with pytest.raises(capi.GvtmError) as err:
        call(*args)
    return err.value.status


def test_modes_refusals_and_the_drift_generators_across_resets():
    plan = audio_plan("f32")
    utterances = stream_utterances()
    ids = [IDS[4], IDS[8], IDS[3]]
    push = [utterances[4][:1], utterances[8][:1], []]
    more = [utterances[4][1:], utterances[8][1:], []]
    frames_in = tracks.random_tracks(3, 2, seed0=11)
    d0 = used_drift(3, seed=9)

    # an undisturbed stream
    calm = g.Stream(plan, 3, voice_ids=ids)
    calm.set_drift(d0)
    calm_first, calm_frames = calm.push_events(push)
    calm_more, _ = calm.push_events(more)
    assert max(s.size for s in calm_more) > 0

    st = g.Stream(plan, 3, voice_ids=ids)
    assert st.get_drift().tobytes() == fresh_drift(3).tobytes()
    st.set_drift(d0)
    assert st.get_drift().tobytes() == d0.tobytes()
    first, new = st.push_events(push)
    assert new.tolist() == calm_frames.tolist() and new[2] == 0 and (new[:2] > 0).all()
    after_first = st.get_drift()
    assert after_first[:2].tobytes() != d0[:2].tobytes() and after_first[2].tobytes() == d0[2].tobytes()
    # one feeding mode per run: frames are refused now, and so is a change of the drift states
    assert status_of(st.push, frames_in) == INVALID_ARGUMENT
    assert status_of(st.set_drift, d0) == INVALID_ARGUMENT
    assert status_of(st.set_drift, None) == INVALID_ARGUMENT
    # an audio_stride one sample short: refused, and the stream is as it was -- drift states, held frames, mode
    need = max(s.size for s in calm_more)
    assert status_of(st.push_events, more, need - 1) == INVALID_ARGUMENT
    assert st.get_drift().tobytes() == after_first.tobytes()
    assert status_of(st.push, frames_in) == INVALID_ARGUMENT
    again, _ = st.push_events(more, need)
    for b in range(3):
        assert first[b].tobytes() == calm_first[b].tobytes() and again[b].tobytes() == calm_more[b].tobytes(), b
    tails, _ = st.finish()
    calm_tails, _ = calm.finish()
    assert all(t.tobytes() == c.tobytes() for t, c in zip(tails, calm_tails))
    assert status_of(st.push_events, more) == INVALID_ARGUMENT  # finished

    # a reset keeps the drift states and opens either mode; set_drift(None) reseeds
    ran = st.get_drift()
    assert ran.tobytes() == calm.get_drift().tobytes() and ran[:2].tobytes() != after_first[:2].tobytes()
    st.reset()
    assert st.get_drift().tobytes() == ran.tobytes()
    st.push(frames_in)
    assert status_of(st.push_events, push) == INVALID_ARGUMENT
    assert st.get_drift().tobytes() == ran.tobytes()
    st.reset(ids)
    assert st.get_drift().tobytes() == ran.tobytes()
    st.set_drift(None)
    assert st.get_drift().tobytes() == fresh_drift(3).tobytes()
    st.push_events(push)

    # a plan without track configurations
    bare = g.VoicesPlan(configs(44100.0, 1, capi.PRECISION_F32), 250.0, 0)
    st = g.Stream(bare, 3, voice_ids=ids)
    assert status_of(st.push_events, push) == INVALID_ARGUMENT
    assert "gvtm_plan_set_voice_tracks" in bare._lib.gvtm_last_error().decode()


# ---- 6. pushes that bring nothing

def test_pushes_without_chunks_and_without_events():
    """A push with a null utt_chunks, one whose utterances receive no chunk and one whose only chunk holds no event: each
    generates no frame, returns no sample and leaves the drift states alone, before the first frames and while frames are
    held; the samples of the run are those of a frames-fed stream given the chained tracks oracle's frames."""
    plan = audio_plan("f32")
    ids = [0, 1, 2]
    chunks = [[make_singable(list_with_frames(c))] for c in (9, 5, 11)]
    assert all(capi.events_from_table(u[0]).shape[0] <= 12 for u in chunks)
    d0 = used_drift(3, seed=21)
    st = g.Stream(plan, 3, voice_ids=ids)
    st.set_drift(d0)

    def push_nothing(how):
        audio, counts, frames = np.full((3, 8), 5.0, np.float32), np.full(3, -1, np.int64), np.full(3, -1, np.int32)
        before = st.get_drift()
        if how == "null":
            plan._check(plan._lib.gvtm_stream_push_events(st._h, None, None, None, capi._ptr(audio), 8, capi._ptr(counts), capi._ptr(frames)))
        else:
            got, frames = st.push_events([[], [], []] if how == "no chunk" else [[], [np.zeros((0, 38))], []])
            counts = np.array([s.size for s in got])
        assert not counts.any() and not frames.any() and st.get_drift().tobytes() == before.tobytes(), how

    for how in ("null", "no chunk", "no event"):
        push_nothing(how)
    first, new = st.push_events(chunks)
    assert new.tolist() == [frame_count(AUDIO_TRACKS[v], u) for v, u in zip(ids, chunks)] == [9, 5, 11]
    for how in ("null", "no chunk", "no event"):  # (rows are held now)
        push_nothing(how)
    tails, maxabs = st.finish()

    fed = g.Stream(plan, 3, voice_ids=ids)
    rows = [chain_oracle(AUDIO_TRACKS[v], u, d0[b])[0] for b, (v, u) in enumerate(zip(ids, chunks))]
    buf = np.zeros((3, 11, 16), dtype=np.float32)
    for b, r in enumerate(rows):
        buf[b, : r.shape[0]] = r
    fed_first = fed.push(buf, np.array([r.shape[0] for r in rows], dtype=np.int32))
    fed_tails, fed_maxabs = fed.finish()
    for b in range(3):
        assert first[b].tobytes() == fed_first[b].tobytes() and tails[b].tobytes() == fed_tails[b].tobytes() and tails[b].size > 0, b
    assert maxabs.tobytes() == fed_maxabs.tobytes()
