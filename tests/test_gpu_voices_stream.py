"""Streams over plans of several voices (gvtm_stream_create_voices / gvtm_stream_reset_voices).

Utterance b of a voices stream must come out, bit for bit (samples, counts, maxabs), as a gvtm_stream_create stream on a
single-voice plan of its voice gives it for the same frames, whatever the split of the pushes, the mix of ids and the
workgroup shape.  The five 0_male variants (tests/golden/voice_*.txt) in every precision, the five 5_male variants
(voice5_*.txt) with their flush-overrun lengths against the reference vectors of tests/golden/voices5_golden.npz."""
import numpy as np
import pytest

import gama_tts_amd as g
from gama_tts_amd import capi
import model5_cases as cases5
import oracle
import tracks
import voice_files
from parity_rules import check_model5
from voice_cases import CASE_IDS, CASES, configs, configs5, oracle_config

pytestmark = pytest.mark.gpu


def ragged_schedule(total, rng, max_piece=25, single_rounds=0):
    """Per-round new frames of each utterance: first `single_rounds` rounds of one frame each, then 0, 1 or up to
    max_piece, until every utterance has its total."""
    total = np.asarray(total, dtype=np.int64)
    at = np.zeros(len(total), dtype=np.int64)
    rounds = []
    for _ in range(single_rounds):
        n = np.minimum(1, total - at).astype(np.int32)
        rounds.append(n)
        at += n
    while (at < total).any():
        kind = rng.integers(0, 4, size=len(total))
        n = np.where(kind == 0, 0, np.where(kind == 1, 1, rng.integers(2, max_piece + 1, size=len(total))))
        n = np.minimum(n, total - at).astype(np.int32)
        rounds.append(n)
        at += n
    return rounds


def lockstep_schedule(total, rng, max_piece=25):
    """Every utterance takes the same frames each round (total equal across the batch)."""
    left, rounds = int(total[0]), []
    while left > 0:
        k = min(int(rng.integers(1, max_piece + 1)), left)
        rounds.append(np.full(len(total), k, dtype=np.int32))
        left -= k
    return rounds


def run_stream(st, params, rounds, cols=None):
    """Pushes rounds[r][cols] of the utterances `cols` of params, then finishes: (per-utterance samples, maxabs)."""
    cols = np.arange(params.shape[0]) if cols is None else np.asarray(cols)
    got = [[] for _ in cols]
    at = np.zeros(len(cols), dtype=np.int64)
    for r in rounds:
        n = r[cols]
        block = np.zeros((len(cols), max(int(n.max()), 1), 16), dtype=np.float32)
        for j, b in enumerate(cols):
            block[j, : n[j]] = params[b, at[j]: at[j] + n[j]]
        for j, piece in enumerate(st.push(block, n)):
            got[j].append(piece)
        at += n
    tails, maxabs = st.finish()
    return [np.concatenate(got[j] + [tails[j]]) for j in range(len(cols))], maxabs


def single_voice_references(cfgs, params, ids, rounds, diagnostics=False, rows=0):
    """Every utterance through a gvtm_stream_create stream on a single-voice plan of its voice: {b: (samples, maxabs)}."""
    out = {}
    for v, cfg in enumerate(cfgs):
        sel = np.nonzero(ids == v)[0]
        if sel.size == 0:
            continue
        plan = g.Plan(cfg, 250.0, 0, diagnostics=diagnostics, rows=rows)
        samples, maxabs = run_stream(g.Stream(plan, sel.size), params, rounds, sel)
        for j, b in enumerate(sel):
            out[int(b)] = (samples[j], float(maxabs[j]))
    return out


def assert_as_singles(samples, maxabs, refs):
    for b, (ref, peak) in refs.items():
        assert samples[b].size == ref.size, b
        assert np.array_equal(samples[b], ref), b
        assert maxabs[b] == peak, b


def overrun_length(plan, voice, lo=1, hi=400):
    """The shortest frame count in [lo, hi) whose output count exceeds that of one frame more (the flush overrun's lap)."""
    for n in range(lo, hi):
        if plan.voice_output_count(voice, n) > plan.voice_output_count(voice, n + 1):
            return n
    return None


@pytest.mark.parametrize("precision,delay,rate,layout", CASES, ids=CASE_IDS)
def test_five_voices_ragged_pushes(precision, delay, rate, layout):
    cfgs = configs(rate, delay, precision, layout)
    plan = g.VoicesPlan(cfgs, 250.0, 0)
    rng = np.random.default_rng(31 + delay + 3 * precision + 7 * layout)
    batch = 15
    ids = rng.permutation(np.repeat(np.arange(5, dtype=np.int32), 3))
    total = rng.integers(0, 41, size=batch).astype(np.int64)
    total[np.nonzero(ids == 2)[0][0]] = 0
    total[np.nonzero(ids == 3)[0][0]] = 1
    # a down-sampling voice ending on a flush-overrun length, where one exists in reach: at 22.05 kHz (layout 1) voice 0
    # overruns at 83 frames and voice 4 at 15; at 44.1 kHz no down-sampling voice overruns below 400 frames, in any case
    overrun = None
    for v in range(5):
        if plan.voice_info(v).upsampling == 0 and overrun_length(plan, v) is not None:
            overrun = (v, overrun_length(plan, v))
            b = int(np.nonzero(ids == v)[0][1])
            total[b] = overrun[1]
            break
    assert (overrun is not None) == (layout == 1), overrun
    params = tracks.random_tracks(batch, int(total.max()), seed0=900 + precision, consonant_heavy=True)
    rounds = ragged_schedule(total, rng, single_rounds=1)
    st = g.Stream(plan, batch, voice_ids=ids)
    samples, maxabs = run_stream(st, params, rounds)
    refs = single_voice_references(cfgs, params, ids, rounds)
    assert_as_singles(samples, maxabs, refs)
    for b in range(batch):
        v = int(ids[b])
        at = sum(int(r[b]) for r in rounds)
        assert samples[b].size == plan.voice_output_count(v, at), b
        if precision == capi.PRECISION_F32:
            want = oracle.synthesize(oracle_config(voice_files.VOICES[v], rate, delay, layout, precision), params[b, :at])
            assert np.array_equal(samples[b], want), (b, v)


@pytest.mark.parametrize("precision", [capi.PRECISION_F32, capi.PRECISION_F64], ids=["f32", "f64"])
def test_lockstep_voices_share_workgroups(precision):
    """All five voices in lockstep through the diagnostics library with four rows: voice 1 has one utterance, voice 3
    five, so some workgroups are partly empty."""
    cfgs = configs(precision=precision)
    plan = g.VoicesPlan(cfgs, 250.0, 0, diagnostics=True, rows=4)
    counts = [2, 1, 4, 5, 3]
    ids = np.random.default_rng(8).permutation(np.repeat(np.arange(5, dtype=np.int32), counts))
    batch = ids.size
    total = np.full(batch, 46, dtype=np.int64)
    params = tracks.random_tracks(batch, 46, seed0=1300, consonant_heavy=True)
    rounds = lockstep_schedule(total, np.random.default_rng(9))
    st = g.Stream(plan, batch, voice_ids=ids)
    samples, maxabs = run_stream(st, params, rounds)
    assert_as_singles(samples, maxabs, single_voice_references(cfgs, params, ids, rounds, diagnostics=True, rows=4))
    # and the same as the one-shot entry (which the single-voice streams already match in their own shapes)
    audio, n, peak = plan.synthesize_host(params, ids)
    for b in range(batch):
        assert n[b] == samples[b].size and np.array_equal(audio[b, : n[b]], samples[b]) and peak[b] == maxabs[b], b


@pytest.mark.parametrize("precision", [capi.PRECISION_MIXED, capi.PRECISION_F64], ids=["mixed", "f64"])
def test_workgroup_shape_changes_between_pushes(precision):
    """One stream whose launches change shape: multi-row launches (lockstep within each voice) and one-row launches (ragged
    within a voice) alternate, and the finish is ragged.  Four up-sampling voices, so that a multi-row shape fits the LDS
    with the one-row shape's ring (mixed: four rows of 32 steps against one of 96; fp64: two rows of 48 against one of 84)
    and the ring that shape would pick for itself (256 samples) is not the stream's (512).  (In float no multi-row shape
    with a ring of its own fits next to the stream's ring: two rows of 96 steps already take 512.)  Every launch must
    keep each voice's ring at its single-voice stream's length, or the state one shape saves is not the one the next
    reads.  References: single-voice streams, whose launches all have one row."""
    names = voice_files.VOICES[:4]
    cfgs = configs(precision=precision, names=names)
    plan = g.VoicesPlan(cfgs, 250.0, 0, diagnostics=True, rows=4)
    for v in range(4):
        assert plan.voice_info(v).upsampling == 1
    ids = np.random.default_rng(12).permutation(np.repeat(np.arange(4, dtype=np.int32), [1, 3, 5, 2]))
    batch = ids.size
    first = np.array([int(np.nonzero(ids == ids[b])[0][0]) == b for b in range(batch)])
    full = lambda k: np.full(batch, k, dtype=np.int32)  # noqa: E731
    rounds = [
        full(10),                                              # lockstep: multi-row
        (3 + 2 * ids).astype(np.int32),                        # lockstep within each voice: multi-row
        np.where(first, 7, 0).astype(np.int32),                # ragged within a voice: one row
        np.where(first, 0, 7).astype(np.int32),                # one row, and the steps done agree again
        full(9),                                               # multi-row
        np.where(np.arange(batch) == 2, 2, 0).astype(np.int32),  # one row; the finish too
    ]
    total = np.sum(rounds, axis=0)
    params = tracks.random_tracks(batch, int(total.max()), seed0=7100 + precision, consonant_heavy=True)
    samples, maxabs = run_stream(g.Stream(plan, batch, voice_ids=ids), params, rounds)
    assert_as_singles(samples, maxabs, single_voice_references(cfgs, params, ids, rounds))
    for b in range(batch):
        assert samples[b].size == plan.voice_output_count(int(ids[b]), int(total[b])), b


@pytest.mark.parametrize("rate", sorted({c["rate"] for c in cases5.CASES["voices5"]}), ids=lambda r: "%dHz" % r)
def test_model5_five_voices_with_overrun_lengths(rate, golden):
    """Ragged and single-frame pushes of all five 5_male voices; the overrun cases of this output rate against the
    reference's vectors."""
    cfgs = configs5(rate)
    plan = g.VoicesPlan(cfgs, 250.0, 0)
    golden5v = cases5.load("voices5")
    sel = [c for c in cases5.CASES["voices5"] if c["rate"] == rate and c["store"] == "tail"]
    trs = [cases5.track_for(c, golden) for c in sel]
    ids = [voice_files.VOICES.index(c["voice"]) for c in sel]
    rng = np.random.default_rng(int(rate))
    for v in range(5):  # two more utterances of every voice
        for _ in range(2):
            trs.append(tracks.random_tracks(1, int(rng.integers(0, 60)), seed0=int(rng.integers(1 << 20)), consonant_heavy=True)[0])
            ids.append(v)
    order = rng.permutation(len(trs))
    trs = [trs[i] for i in order]
    ids = np.array([ids[i] for i in order], dtype=np.int32)
    total = np.array([t.shape[0] for t in trs], dtype=np.int64)
    params = np.zeros((len(trs), int(total.max()), 16), dtype=np.float32)
    for b, t in enumerate(trs):
        params[b, : t.shape[0]] = t
    rounds = ragged_schedule(total, rng, max_piece=120, single_rounds=3)
    samples, maxabs = run_stream(g.Stream(plan, len(trs), voice_ids=ids), params, rounds)
    assert_as_singles(samples, maxabs, single_voice_references(cfgs, params, ids, rounds))
    for i, c in enumerate(sel):
        b = int(np.nonzero(order == i)[0][0])
        m = golden5v["manifest"][c["name"]]
        out = samples[b]
        assert out.size == m["n"], c["name"]
        for got, key in cases5.stored(c, out):
            check_model5(got, golden5v[key], peak=m["maxabs"])
        assert maxabs[b] == pytest.approx(m["maxabs"], rel=1e-5)


@pytest.mark.parametrize("model5", [False, True], ids=["v2", "model5"])
def test_reset_voices_gives_the_new_voices(model5):
    cfgs = configs5() if model5 else configs(precision=capi.PRECISION_F32)
    plan = g.VoicesPlan(cfgs, 250.0, 0)
    ids = np.array([0, 1, 2, 3, 4, 0], dtype=np.int32)
    batch = ids.size
    params = tracks.random_tracks(batch, 30, seed0=4242, consonant_heavy=True)
    rng = np.random.default_rng(77)
    rounds = ragged_schedule(np.full(batch, 30, dtype=np.int64), rng, max_piece=12)
    st = g.Stream(plan, batch, voice_ids=ids)
    first, first_max = run_stream(st, params, rounds)
    assert_as_singles(first, first_max, single_voice_references(cfgs, params, ids, rounds))
    # reset() keeps the ids: the same samples again
    st.reset()
    again, again_max = run_stream(st, params, rounds)
    for b in range(batch):
        assert np.array_equal(again[b], first[b]) and again_max[b] == first_max[b], b
    # a refused reset_voices leaves the stream as it was (finished: a push is refused until a reset)
    with pytest.raises(capi.GvtmError) as e:
        st.reset([0, 1, 2, 3, 4, 5])
    assert e.value.status == 1 and "utterance 5" in str(e.value)
    with pytest.raises(capi.GvtmError):
        st.push(params[:, :1])
    perm = np.array([4, 3, 0, 1, 2, 2], dtype=np.int32)
    st.reset(perm)
    moved, moved_max = run_stream(st, params, rounds)
    assert_as_singles(moved, moved_max, single_voice_references(cfgs, params, perm, rounds))
    assert moved[0].size != first[0].size or not np.array_equal(moved[0], first[0])  # voice 4 now, not voice 0


@pytest.mark.parametrize("model5", [False, True], ids=["v2", "model5"])
def test_one_voice_plan_with_zero_ids_is_the_plain_stream(model5):
    cfg = configs5(names=["female"])[0] if model5 else configs(precision=capi.PRECISION_F64, names=["small_child"])[0]
    params = tracks.random_tracks(4, 40, seed0=515, consonant_heavy=True)
    rounds = ragged_schedule(np.array([40, 0, 17, 40]), np.random.default_rng(2), max_piece=10)
    plain = g.Plan(cfg, 250.0, 0)
    want, want_max = run_stream(g.Stream(plain, 4), params, rounds)
    for plan in (g.VoicesPlan([cfg], 250.0, 0), plain):
        got, got_max = run_stream(g.Stream(plan, 4, voice_ids=np.zeros(4, dtype=np.int32)), params, rounds)
        for b in range(4):
            assert np.array_equal(got[b], want[b]) and got_max[b] == want_max[b], b


def test_a_refused_push_leaves_the_stream_as_it_was():
    cfgs = configs(precision=capi.PRECISION_MIXED)
    plan = g.VoicesPlan(cfgs, 250.0, 0)
    ids = np.array([4, 0, 2, 1, 3], dtype=np.int32)
    params = tracks.random_tracks(5, 36, seed0=99, consonant_heavy=True)
    lib = plan._lib
    st = g.Stream(plan, 5, voice_ids=ids)
    head = np.ascontiguousarray(params[:, :20])
    stride = st.capacity(20)
    audio = np.zeros((5, stride), dtype=np.float32)
    counts = np.zeros(5, dtype=np.int64)
    # a stride too small for what the push produces: refused, nothing synthesized, nothing kept
    assert lib.gvtm_stream_push(st._h, head.ctypes.data, None, 20, audio.ctypes.data, 8, counts.ctypes.data) == 1
    assert b"audio_stride" in lib.gvtm_last_error()
    pieces = st.push(head)
    rest = st.push(params[:, 20:])
    tails, maxabs = st.finish()
    rounds = [np.full(5, 20, dtype=np.int32), np.full(5, 16, dtype=np.int32)]
    refs = single_voice_references(cfgs, params, ids, rounds)
    assert_as_singles([np.concatenate([pieces[b], rest[b], tails[b]]) for b in range(5)], maxabs, refs)
