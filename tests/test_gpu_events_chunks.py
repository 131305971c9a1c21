"""Utterances of several event lists in one launch (gvtm_generate_tracks_chunks_device,
gvtm_synthesize_events_chunks_device; vtm_tracks_kernel<TrackChunksArgs>).

The reference builds an utterance from one generateOutput() call per /c chunk of the phonetic string, all on one parameter
list and with one drift generator running on (Controller.cpp:141-154).  So an utterance's frames must be, bit for bit, the
chunks' frames one after the other, each chunk generated as a list of its own with the drift state the chunk before left:
against the reference's own chained calls (tracks_golden.npz, calls 0 and 1 of each text), against the chained tracks
oracle, and, with one chunk per utterance, against gvtm_generate_tracks_voices_device.  The events-to-audio entry must equal
the two calls it stands for and, in float, the float oracle on the concatenated frames."""
import numpy as np
import pytest

from gama_tts_amd import capi
import event_lists
import oracle
from chunk_cases import (DIVERSE_TRACKS, VARIANT_TRACKS, boundary_list, chain_oracle, check_rows, generate_tracks_chunks,
                         list_with_frames, offset_tables, random_list, synthesize_chunks)
from device_io import generate_tracks
from track_cases import fresh_drift, product_config, singable_event_table, used_drift
from voice_cases import configs
from voices5_float_cases import float_voices_plan

import gama_tts_amd as g

pytestmark = pytest.mark.gpu

BAD_VOICE = 7


def voices_plan(cfgs, cfgvs):
    plan = g.VoicesPlan(cfgs, 250.0, 0)
    plan.set_voice_tracks([product_config(c) for c in cfgvs])
    return plan


def frame_count(cfgv, chunks):
    events, chunk_offsets, _ = offset_tables([chunks])
    return capi.tracks_chunks_frame_count(product_config(cfgv), events, chunk_offsets)


def oracle_rows(cfgvs, utterances, ids, drift0, cache=None):
    return [chain_oracle(cfgvs[v], u, drift0[b], cache) if 0 <= v < len(cfgvs) else None for b, (u, v) in enumerate(zip(utterances, ids))]


# ---- 1. pinned to the reference directly

def test_two_captured_reference_calls_are_one_utterance_of_two_chunks(golden_tracks):
    calls = {name: [event_lists.load_golden(golden_tracks, name, c) for c in (0, 1)] for name in event_lists.CAPTURED}
    cfg0 = calls["hello"][0][0]
    for name, ((cfg_a, events_a, frames_a), (cfg_b, events_b, frames_b)) in calls.items():
        # the same list under the same configuration, twice; what differs is what the carried drift state makes
        assert np.array_equal(cfg_a, cfg_b) and np.array_equal(cfg_a, cfg0) and np.array_equal(events_a, events_b), name
        assert frames_a.shape == frames_b.shape and not np.array_equal(frames_a, frames_b), name
        assert not np.isnan(frames_a).any() and not np.isnan(frames_b).any()
    assert [calls[n][0][2].shape[0] for n in event_lists.CAPTURED] == [332, 875, 375, 675]
    cfgvs = []
    for shift in (-12.0, -3.0, 0.0, 2.5, 7.0):  # voice 2: the captured configuration; the rest: other mean pitches
        c = np.array(cfg0, dtype=np.float64)
        c[6] += shift
        cfgvs.append(c)
    plan = voices_plan(configs(precision=capi.PRECISION_F32), cfgvs)
    utterances, ids = [], []
    for q, name in enumerate(event_lists.CAPTURED):  # the two-chunk utterance, call 0 alone, and the two chunks under another voice
        events = calls[name][0][1]
        utterances += [[events, events], [events], [events, events]]
        ids += [2, 2, [0, 1, 3, 4][q]]
    batch = len(utterances)
    drift0 = fresh_drift(batch)
    max_frames = 2 * 875 + 3
    got = generate_tracks_chunks(plan, utterances, ids, max_frames, drift0)
    want = []
    for q, name in enumerate(event_lists.CAPTURED):
        (_, events, frames_a), (_, _, frames_b) = calls[name]
        state_a = oracle.tracks_generate(oracle.track_config(cfg0), events)[1]
        state_b = oracle.tracks_generate(oracle.track_config(cfg0), events, state_a)[1]
        want += [(np.concatenate([frames_a, frames_b]), state_b), (frames_a, state_a),
                 chain_oracle(cfgvs[ids[3 * q + 2]], [events, events], drift0[3 * q + 2])]
    check_rows(got, want, max_frames, drift0, "captured")
    params, _, counts, _ = got
    for q in range(len(event_lists.CAPTURED)):
        n = int(counts[3 * q])
        assert counts[3 * q + 2] == n == 2 * counts[3 * q + 1]
        assert not np.array_equal(params[3 * q + 2, :n, 0], params[3 * q, :n, 0])  # another mean pitch


# ---- 2. the chained oracle, five voices

def edge_batch():
    """-> (utterances, ids): 0, 1, 2, 3 and 7 chunks; chunks of 0 / 1 / 2 events as first, middle and last chunk; tabled
    chunks (240 events) in front of and behind untabled ones (241, 260); chunks of exactly 1, 31, 32 and 33 frames, which put
    chunk boundaries at frames 1, 32, 64, 97 resp. 31, 32, 65 of their utterance: before, on and behind a flush of the
    32-frame ring; one row with a voice id outside the table; an odd batch, so that the last workgroup holds one row."""
    L = random_list
    e0, e1, e2 = (boundary_list(n, seed=50 + n) for n in (0, 1, 2))
    t240, t240b, t241, t260 = boundary_list(240, seed=1), L(240, 240), boundary_list(241, seed=2), L(260, 260)
    f1, f31, f32, f33 = (list_with_frames(c) for c in (1, 31, 32, 33))
    utterances = [[],
                  [L(100, 40)],
                  [L(101, 17), L(102, 33)],
                  [e0, L(103, 40), e1, L(104, 17), e2],
                  [e1, L(105, 9), e2, L(106, 25), e0],
                  [e2, L(107, 33), e0, L(108, 3), e1],
                  [t240, t241, t260, t240b],
                  [f1, f31, f32, f33, L(109, 40), f33, f1],
                  [f31, f1, f33],
                  [L(110, 40), L(111, 17)],
                  [t241, t240]]
    ids = [b % 5 for b in range(len(utterances))]
    ids[9] = BAD_VOICE
    assert len(utterances) % 2 == 1 and sorted({len(u) for u in utterances}) == [0, 1, 2, 3, 4, 5, 7]
    return utterances, ids


def test_chunks_against_the_chained_oracle_and_cut_by_max_frames():
    utterances, ids = edge_batch()
    batch = len(utterances)
    drift0 = used_drift(batch)
    want = oracle_rows(DIVERSE_TRACKS, utterances, ids, drift0)
    assert want[9] is None and want[0][0].shape[0] == 0
    assert [oracle.tracks_generate(oracle.track_config(DIVERSE_TRACKS[0]), t)[0].shape[0] for t in utterances[7][:4]] == [1, 31, 32, 33]
    plan = voices_plan(configs(precision=capi.PRECISION_F32), DIVERSE_TRACKS)
    max_frames = max(w[0].shape[0] for w in want if w)
    check_rows(generate_tracks_chunks(plan, utterances, ids, max_frames, drift0), want, max_frames, drift0, "whole")
    # the host's count agrees
    assert [frame_count(DIVERSE_TRACKS[v], u) for u, v in zip(utterances, ids) if v != BAD_VOICE] == [w[0].shape[0] for w in want if w]
    # rows shorter than the utterances: cut inside a first chunk, exactly at a chunk boundary and inside a later chunk (of
    # utterance 2; the others are cut wherever that falls); counts and drift states are still those of the whole utterances
    first = frame_count(DIVERSE_TRACKS[ids[2]], utterances[2][:1])
    assert 5 < first < want[2][0].shape[0] - 7
    for cut in (first - 5, first, first + 7):
        check_rows(generate_tracks_chunks(plan, utterances, ids, cut, drift0), want, cut, drift0, "cut at %d" % cut)


# ---- 3. one chunk per utterance: the voices entry

def test_one_chunk_per_utterance_equals_the_voices_entry():
    lengths = [40, 2, 1, 17, 80, 3, 55, 9, 33, 110, 0, 150, 260, 239, 240, 241]
    tables = [random_list(100 + b, n) for b, n in enumerate(lengths)]
    ids = [b % 5 for b in range(len(tables))]
    tables.insert(6, random_list(99, 40))
    ids.insert(6, BAD_VOICE)
    batch = len(tables)
    assert batch % 2 == 1
    drift0 = used_drift(batch)
    plan = voices_plan(configs(precision=capi.PRECISION_F32), DIVERSE_TRACKS)
    max_frames = max(capi.tracks_frame_count(product_config(DIVERSE_TRACKS[0]), capi.events_from_table(t)) for t in tables)
    v_params, v_counts, v_drift = generate_tracks(tables, max_frames, drift0, plan=plan, ids=ids)
    params, _, counts, drift = generate_tracks_chunks(plan, [[t] for t in tables], ids, max_frames, drift0)
    assert counts.tobytes() == v_counts.tobytes() and (counts > 0).sum() >= 12 and counts[6] == 0
    assert drift.tobytes() == v_drift.tobytes()
    for b in range(batch):
        n = int(counts[b])
        assert params[b, :n].tobytes() == v_params[b, :n].tobytes(), b


# ---- 4. a batch of 1,025

def test_batch_of_1025():
    """1,025 utterances of 1 to 5 chunks drawn from the lists of the edge batch, five voices, three drift states, rows of 600
    frames: every row against the chained oracle."""
    pool = []
    for u in edge_batch()[0]:
        pool += [t for t in u if not any(t is p for p in pool)]
    rng = np.random.default_rng(1025)
    batch = 1025
    utterances = [[pool[k] for k in rng.integers(0, len(pool), rng.integers(1, 6))] for _ in range(batch)]
    ids = rng.integers(0, 5, batch)
    drift0 = used_drift(3)[rng.integers(0, 3, batch)]
    want = oracle_rows(DIVERSE_TRACKS, utterances, ids, drift0, cache={})
    assert sum(1 for w in want if w[0].shape[0] > 600) > 100 and sum(1 for w in want if 0 < w[0].shape[0] < 600) > 100
    plan = voices_plan(configs(precision=capi.PRECISION_F32), DIVERSE_TRACKS)
    check_rows(generate_tracks_chunks(plan, utterances, ids, 600, drift0), want, 600, drift0, "batch 1025")


# ---- 5. events to audio

SINGABLE = [(300, 40), (301, 2), (302, 1), (303, 17), (305, 3), (306, 55), (307, 9), (308, 33), (309, 25)]
# voice 0 (male) without macro intonation: the utterances that go against the float oracle
ORACLE_TRACK = np.array([4, 0, 1, 1, 1, -20.0, -16.0, 4.0, 250.0, 4.0])
AUDIO_TRACKS = [ORACLE_TRACK] + VARIANT_TRACKS[1:]


def singable_utterances():
    """-> (utterances, ids): rows 0 and 1 the two oracle utterances (voice 0), then utterances of 0 to 3 chunks of every voice."""
    S = {sn: singable_event_table(*sn) for sn in SINGABLE}
    utterances = [[S[300, 40], S[303, 17], S[306, 55]],
                  [S[308, 33], S[309, 25], S[300, 40], S[303, 17]],
                  [S[306, 55]], [], [S[301, 2], S[307, 9]], [S[302, 1], S[305, 3], S[303, 17]], [S[309, 25], S[308, 33]],
                  [S[300, 40]], [S[307, 9], S[302, 1], S[305, 3]]]
    ids = [0, 0, 1, 2, 3, 4, 0, 1, 2]
    return utterances, ids


def audio_plan(kind):
    if kind == "model5_f32":
        plan = float_voices_plan(rate=48000.0)
        plan.set_voice_tracks([product_config(c) for c in AUDIO_TRACKS])
        return plan
    return voices_plan(configs(44100.0, 1, capi.PRECISION_F32 if kind == "f32" else capi.PRECISION_F64), AUDIO_TRACKS)


@pytest.mark.parametrize("kind", ["f32", "f64", "model5_f32"])
def test_events_entry_equals_the_two_calls_and_the_float_oracle(kind):
    utterances, ids = singable_utterances()
    batch = len(utterances)
    assert batch % 2 == 1
    frames_of = [frame_count(AUDIO_TRACKS[v], u) for u, v in zip(utterances, ids)]
    assert frames_of[:2] == [673, 702] and frames_of[3] == 0
    max_frames = max(frames_of)
    plan = audio_plan(kind)
    stride = plan.voices_output_capacity(max_frames)
    drift0 = fresh_drift(batch)
    entry = synthesize_chunks(plan, utterances, ids, max_frames, stride, drift0, entry=True)
    chain = synthesize_chunks(plan, utterances, ids, max_frames, stride, drift0, entry=False)
    assert entry["frames"].tolist() == frames_of and (entry["counts"][np.array(frames_of) > 0] > 0).all()
    for key in chain:  # samples, frame counts, sample counts, peaks, drift states
        assert entry[key].dtype == chain[key].dtype and entry[key].tobytes() == chain[key].tobytes(), key
    if kind != "f32":
        return
    # bit identity is the float path's contract: the float oracle on the chained tracks oracle's frames
    for b, samples in ((0, 118574), (1, 123681)):
        frames, state = chain_oracle(ORACLE_TRACK, utterances[b], drift0[b])
        assert frames.shape[0] == frames_of[b]
        ref = oracle.synthesize(oracle.male_config(44100.0, 1, float_model=1), frames)
        assert ref.size == samples and np.isfinite(ref).all()
        assert entry["counts"][b] == ref.size
        assert entry["audio"][b, : ref.size].tobytes() == ref.tobytes(), b
        assert not entry["audio"][b, ref.size:].any()
        assert entry["drift"][b].tobytes() == np.array(state, dtype=np.float64).tobytes()
