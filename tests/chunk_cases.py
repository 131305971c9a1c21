"""Utterances of several event lists (gvtm_generate_tracks_chunks_device, gvtm_synthesize_events_chunks_device): an
utterance is a list of event tables ("chunks"), a batch a list of utterances.  The two offset tables of a batch, the chained
tracks oracle (one oracle call per chunk, each call's drift state the next one's, frames concatenated: what the reference's
loop over the /c chunks does, Controller.cpp:141-154), and the device calls on pre-filled buffers.  torch is imported inside
the functions: collecting the tests needs no GPU."""
import numpy as np

from gama_tts_amd import capi
import event_lists
import oracle
from device_io import current_stream, filled, to_device, to_host

SENTINEL = 0x7FC0DEAD  # a quiet NaN that marks frames the kernel must not write
GUARD_FRAMES = 64

# the ten numbers of a track configuration (oracle.track_config).  Five that differ in everything a voice may: one each
# with drift, macro, micro and smooth intonation off
DIVERSE_TRACKS = [np.array([4, 1, 1, 1, 1, -20.0, -16.0, 4.0, 250.0, 4.0]),
                  np.array([4, 1, 1, 0, 1, -18.0, -4.0, 3.0, 250.0, 4.0]),
                  np.array([4, 0, 1, 1, 1, -20.0, -1.5, 5.0, 250.0, 6.0]),
                  np.array([4, 1, 0, 1, 1, -22.5, 1.0, 2.0, 250.0, 3.0]),
                  np.array([4, 1, 1, 1, 0, -15.0, 3.5, 4.0, 200.0, 4.0])]
# the five variants of 0_male: mean pitch = -4 + reference_glottal_pitch
VARIANT_TRACKS = [np.array([4, 1, 1, 1, 1, -20.0, mean, 4.0, 250.0, 4.0]) for mean in (-16.0, -4.0, -1.5, 1.0, 3.5)]


def offset_tables(utterances):
    """-> (gvtm_event records of every chunk back to back, chunk_offsets int64 [chunks + 1], utt_chunks int64 [batch + 1])"""
    chunks = [capi.events_from_table(t) for u in utterances for t in u]
    chunk_offsets = np.zeros(len(chunks) + 1, dtype=np.int64)
    chunk_offsets[1:] = np.cumsum([len(c) for c in chunks])
    utt_chunks = np.zeros(len(utterances) + 1, dtype=np.int64)
    utt_chunks[1:] = np.cumsum([len(u) for u in utterances])
    events = np.concatenate(chunks) if chunks else np.zeros(0, dtype=capi.EVENT_DTYPE)
    return events, chunk_offsets, utt_chunks


def chunks_on_device(utterances):
    """offset_tables on the device (the records as bytes; one spare record, so that a batch without events still has a buffer)."""
    events, chunk_offsets, utt_chunks = offset_tables(utterances)
    events = np.concatenate([events, np.zeros(1, dtype=capi.EVENT_DTYPE)])
    return to_device(events.view(np.uint8), chunk_offsets, utt_chunks)


def starts_plain(t):
    """The event table t with no macro-intonation polynomial on an event at time 0.  generateOutput() divides by the time of
    the first event that carries one (EventList.cpp:966-979): at time 0 the slope is infinite and frame 0's pitch 0 * inf, a
    NaN in the reference as here -- and NaN bits are the one thing the device and the host do not share.  (The parser's
    lists never put one there.)"""
    if t.shape[0] and t[0, 0] == 0:
        t[0, 1] = 0.0
    return t


def random_list(seed, n_events):
    return starts_plain(event_lists.random_event_table(seed, n_events=n_events))


def boundary_list(n_events, seed):
    return starts_plain(event_lists.boundary_table(n_events, seed=seed))


def list_with_frames(count, cp=4):
    """A list that yields exactly `count` frames at control period cp: times on the grid, the last at count periods."""
    n = min(count, 6) + 1
    t = event_lists.random_event_table(4000 + count, n_events=n, control_period=cp)
    steps = np.linspace(0, count, n).round().astype(np.int64)
    steps[-1] = count
    t[:, 0] = cp * steps
    return starts_plain(t)


def chain_oracle(cfgv, chunks, drift, cache=None):
    """The oracle's frames of an utterance and the drift state it leaves: oracle.tracks_generate per chunk under the ten
    numbers cfgv, the state handed on.  cache: {(configuration, id(table), state in): (frames, state out)}, for batches that
    draw their chunks from a pool (the tables must stay alive and unchanged).  The frames are asserted NaN-free: they are
    compared as plain bits."""
    cfg = oracle.track_config(cfgv)
    state = tuple(float(x) for x in drift)
    parts = []
    for t in chunks:
        key = (tuple(cfgv), id(t), state)
        if cache is not None and key in cache:
            frames, state = cache[key]
        else:
            frames, state = oracle.tracks_generate(cfg, t, state)
            assert not np.isnan(frames).any()
            if cache is not None:
                cache[key] = (frames, state)
        parts.append(frames)
    return (np.concatenate(parts) if parts else np.zeros((0, 16), dtype=np.float32)), state


def generate_tracks_chunks(plan, utterances, ids, max_frames, drift0):
    """gvtm_generate_tracks_chunks_device on frames filled with SENTINEL (GUARD_FRAMES more behind the last row) and counts
    filled with 99 -> (params [B][max_frames][16], guard, counts, drift states after), on the host."""
    import torch
    batch = len(utterances)
    d_events, d_chunk_offsets, d_utt_chunks = chunks_on_device(utterances)
    d_ids, d_drift = to_device(np.asarray(ids, dtype=np.int32), np.ascontiguousarray(drift0, dtype=np.float64).copy())
    buf = torch.full(((batch * max_frames + GUARD_FRAMES) * 16,), SENTINEL, dtype=torch.int32, device=d_events.device).view(torch.float32)
    d_counts = filled(batch, 99, np.int32)
    plan.generate_tracks_chunks_device(d_events, d_chunk_offsets, d_utt_chunks, d_ids, batch, max_frames, buf, d_counts, d_drift, current_stream())
    out, counts, drift = to_host(buf, d_counts, d_drift)
    return out[: batch * max_frames * 16].reshape(batch, max_frames, 16), out[batch * max_frames * 16:], counts, drift


def check_rows(got, want, max_frames, drift0, what):
    """got: generate_tracks_chunks' result; want[b]: (frames, state) of the chained oracle, or None for a row the kernel must
    leave alone (a bad voice id: count 0, row and drift state untouched).  Counts in full, frames [0, min(count, max_frames))
    bit for bit, SENTINEL behind them and in the guard, drift states bit for bit."""
    params, guard, counts, drift = got
    assert (guard.view(np.uint32) == SENTINEL).all(), "%s: written past the last row" % what
    for b, w in enumerate(want):
        if w is None:
            assert counts[b] == 0, (what, b)
            assert (params[b].view(np.uint32) == SENTINEL).all(), (what, b)
            assert drift[b].tobytes() == np.asarray(drift0[b], dtype=np.float64).tobytes(), (what, b)
            continue
        frames, state = w
        assert counts[b] == frames.shape[0], (what, b, int(counts[b]), frames.shape[0])
        n = min(frames.shape[0], max_frames)
        assert np.array_equal(params[b, :n].view(np.uint32), frames[:n].view(np.uint32)), (what, b)
        assert (params[b, n:].view(np.uint32) == SENTINEL).all(), (what, b)
        assert drift[b].tobytes() == np.array(state, dtype=np.float64).tobytes(), (what, b)


def synthesize_chunks(plan, utterances, ids, max_frames, stride, drift0, entry):
    """entry=True: gvtm_synthesize_events_chunks_device; False: gvtm_generate_tracks_chunks_device into a buffer of the
    test's, then gvtm_synthesize_voices_device on its frames and counts -> dict of audio [B][stride], frames, counts,
    maxabs, drift on the host; the audio starts out zero, frames and counts 99, maxabs 5.0."""
    batch = len(utterances)
    d_events, d_chunk_offsets, d_utt_chunks = chunks_on_device(utterances)
    d_ids, = to_device(np.asarray(ids, dtype=np.int32))
    out = dict(audio=filled((batch, stride), 0.0, np.float32), frames=filled(batch, 99, np.int32), counts=filled(batch, 99, np.int64),
               maxabs=filled(batch, 5.0, np.float32), drift=to_device(np.ascontiguousarray(drift0, dtype=np.float64).copy())[0])
    if entry:
        plan.synthesize_events_chunks_device(d_events, d_chunk_offsets, d_utt_chunks, d_ids, batch, max_frames, out["audio"], stride,
                                             out["frames"], out["counts"], out["maxabs"], out["drift"], current_stream())
    else:
        d_params = filled((batch, max_frames, 16), 0.0, np.float32)
        plan.generate_tracks_chunks_device(d_events, d_chunk_offsets, d_utt_chunks, d_ids, batch, max_frames, d_params, out["frames"],
                                           out["drift"], current_stream())
        plan.synthesize_voices_device(d_params, d_ids, batch, max_frames, out["audio"], stride, out["frames"], out["counts"],
                                      out["maxabs"], current_stream())
    return dict(zip(out, to_host(*out.values())))
