"""Several voices of the float class of reference model 5 in one launch (gvtm_plan_create_model5_float_voices +
gvtm_synthesize_voices_*, streams and event lists; csrc/vtm_kernels_m5fv.hip).

The five 5_male variants (242 to 564 internal steps per frame) mixed in one batch.  The bar is the float class's:
parity_rules.within(got, ref, TOL[PRECISION_F32]) -- bit identity -- with counts exact and maxabs == abs(out).max().
References: the single-voice float plan of each voice (gvtm_plan_create_model5_float), the float oracle, and the vectors
of the real class (voices5f_golden.npz, vtm5_golden.npz, vtm5f_golden.npz).  "Both shapes": the shape the product picks
(chunk 60 up to 256 utterances, chunk 56 beyond) and a diagnostics plan with rows 2 = chunk 56."""
import hashlib

import numpy as np
import pytest

import gama_tts_amd as g
from gama_tts_amd import capi
import model5_cases as cases
import oracle
import tracks
from device_io import run_voices_device, synthesize_events
from parity_rules import within
from track_cases import fresh_drift, singable_event_table
from voice_cases import mixed_batch, padded, track_configs
from voice_files import VOICES
from voices5_float_cases import BIT_IDENTICAL, assert_as_singles, configs5f, float_voices_plan, single_float_plan, singles_of

pytestmark = pytest.mark.gpu

SHAPES = pytest.mark.parametrize("rows", [0, 2], ids=["product_shape", "chunk56"])

# the (seed, events) pairs of test_gpu_events_voices.py: lists every voice and model can sing (model 5 at 48 kHz included)
SINGABLE = [(300, 40), (301, 2), (302, 1), (303, 17), (305, 3), (306, 55), (307, 9), (308, 33), (309, 25)]

_plans, _shared = {}, {}


def plan_of(rate=cases.RATE, rows=0):
    """The five-voice float plan at `rate` (rows 2: a diagnostics plan forced to chunk 56), made once."""
    if (rate, rows) not in _plans:
        _plans[rate, rows] = float_voices_plan(rate=rate, rows=rows)
    return _plans[rate, rows]


def shared(key, make):
    """A reference computed once and shared by the shapes; its arrays are read-only."""
    if key not in _shared:
        _shared[key] = make()
    return _shared[key]


def oracle_ref(name, rate, track):
    ref, _ = oracle.synthesize5(cases.voice_oracle_config(name, rate, float_model=1), track)
    ref.setflags(write=False)
    return ref


def check_vector(case, out, count, peak, golden):
    """An utterance against a vector of the real class: count, SHA-256, the stored samples, maxabs."""
    data = cases.load(case["fixture"])
    m = data["manifest"][case["name"]]
    assert count == m["n"], case["name"]
    out = out[: m["n"]]
    assert hashlib.sha256(out.tobytes()).hexdigest() == m["sha256"], case["name"]
    for got, key in cases.stored(case, out):
        assert within(got, data[key], BIT_IDENTICAL), key
    assert peak == np.abs(out).max() == np.float32(m["maxabs"]), case["name"]


# ---- 1. five voices in one launch ------------------------------------------------------------------------------------------

@SHAPES
def test_five_voices_in_one_launch(rows):
    cfgs = configs5f()
    plan = plan_of(rows=rows)
    assert plan.n_voices == 5 and all(plan.voice_info(v).precision == capi.PRECISION_F32 for v in range(5))
    params, ids, frames = mixed_batch(45, 14, 5, seed=61)
    audio, counts, maxabs = run_voices_device(plan, params, ids, frames, plan.voices_output_capacity(14))
    for b in range(len(ids)):
        assert counts[b] == plan.voice_output_count(int(ids[b]), int(frames[b]))
    assert_as_singles(audio, counts, maxabs, shared("five", lambda: singles_of(cfgs, params, ids, frames)), ids)
    # the two longest utterances of every voice against the float oracle
    for v, name in enumerate(VOICES):
        sel = np.nonzero(ids == v)[0]
        for b in sel[np.argsort(frames[sel])[-2:]]:
            ref = shared(("five_oracle", int(b)), lambda: oracle_ref(name, cases.RATE, params[b, : frames[b]]))
            assert counts[b] == ref.size and within(audio[b, : ref.size], ref, BIT_IDENTICAL), (name, int(b))


# ---- 2. more than 256 utterances -----------------------------------------------------------------------------------------

def test_more_than_256_utterances_take_the_chunk_56_voice_variant():
    """300 utterances, nothing forced: 300 + 5 one-utterance workgroups of the chunk-56 shape, two per compute unit, the
    five past the last voice's exiting at once."""
    lib = g.load_library(diagnostics=True)
    probe = g.VoicesPlan(configs5f(), 250.0, capi.DEVICE_NONE, diagnostics=True, float_model5=True)
    import ctypes
    out = (ctypes.c_size_t * 3)()
    assert lib.gvtm_debug_launch_shape(probe._h, 300, 1, out) == 0 and (out[0], out[2]) == (1, 80800)
    plan = plan_of()
    params, ids, frames = mixed_batch(300, 6, 5, seed=62)
    audio, counts, maxabs = run_voices_device(plan, params, ids, frames, plan.voices_output_capacity(6))
    assert_as_singles(audio, counts, maxabs, singles_of(configs5f(), params, ids, frames), ids)


# ---- 3. reference vectors through a mixed launch ---------------------------------------------------------------------------

@SHAPES
@pytest.mark.parametrize("rate", sorted({c["rate"] for c in cases.VOICE_CASES}), ids=lambda r: "%dHz" % r)
def test_reference_vectors_through_a_mixed_launch(rate, rows, golden):
    """Every float voice vector of this output rate in one batch (hello, 120 consonant-heavy frames and the flush-overrun
    length of female, large_child, small_child and baby) with a male utterance in between: at 48 kHz the male float vector
    rand5_m5f, at 44.1 kHz a random one held to the oracle."""
    sel = [c for c in cases.VOICE_CASES if c["rate"] == rate]
    male_case = cases.by_name("rand5_m5f") if rate == cases.RATE else None
    male = cases.track_for(male_case or dict(track=("random", 60, 70, True)), golden)
    at = len(sel) // 2
    trs = [cases.track_for(c, golden) for c in sel]
    trs.insert(at, male)
    case_of = list(sel)
    case_of.insert(at, male_case)
    ids = np.array([0 if c is None else VOICES.index(c["voice"]) for c in case_of], dtype=np.int32)
    params, frames = padded(trs)
    plan = plan_of(rate, rows)
    audio, counts, maxabs = plan.synthesize_host(params, ids, frames)
    for b, c in enumerate(case_of):
        if c is not None:
            check_vector(c, audio[b], counts[b], maxabs[b], golden)
            if "ovr" in c["name"]:  # the voice variant's flush-overrun epilogue
                assert counts[b] > plan.voice_output_count(int(ids[b]), int(frames[b]) + 1)
    if male_case is None:
        ref = shared(("male_filler", rate), lambda: oracle_ref("male", rate, male))
        assert counts[at] == ref.size and within(audio[at, : ref.size], ref, BIT_IDENTICAL)
        assert maxabs[at] == np.abs(ref).max()


# ---- 4. voices that differ in the class's switches -------------------------------------------------------------------------

SWITCH_CASES = ["bypass_m5f", "constant_mouth_m5f", "sine_m5f", "no_modulation_m5f", "rand5_m5f"]


@SHAPES
def test_voices_that_differ_in_the_switches_of_the_class(rows, golden):
    """bypass, a constant mouth impedance, the sine source, no noise modulation and the plain male voice: one plan, one
    launch, the same track on every voice, each against the real class's vector for that switch."""
    switch = [cases.by_name(n) for n in SWITCH_CASES]
    assert all(c["track"] == ("random", 120, 5, True) and c["rate"] == cases.RATE and c["float_model"] for c in switch)
    cfgs = configs5f(names=["male"] * 5, overrides={v: c["overrides"] for v, c in enumerate(switch)})
    assert (cfgs[0].bypass, cfgs[1].constant_radius_mouth_impedance, cfgs[2].waveform, cfgs[3].noise_modulation) == (1, 1, 1, 0)
    assert cfgs[1].mouth_impedance_radius == 1.2
    plan = float_voices_plan(cfgs, rows=rows)
    track = cases.track_for(switch[0], golden)
    ids = np.arange(5, dtype=np.int32)
    audio, counts, maxabs = plan.synthesize_host(np.repeat(track[None], 5, axis=0), ids)
    for v, c in enumerate(switch):
        check_vector(c, audio[v], counts[v], maxabs[v], golden)


# ---- 5. one voice only ---------------------------------------------------------------------------------------------------

def test_a_batch_of_one_voice_only():
    plan = plan_of()
    params, _, frames = mixed_batch(20, 10, 5, seed=64)
    ids = np.full(20, 4, dtype=np.int32)  # baby: 564 steps per frame
    audio, counts, maxabs = run_voices_device(plan, params, ids, frames, plan.voices_output_capacity(10))
    assert_as_singles(audio, counts, maxabs, singles_of(configs5f(), params, ids, frames), ids)


def test_one_voice_plan_takes_the_voices_entries_and_the_single_voice_entries():
    cfg = configs5f(names=["small_child"])
    params, _, frames = mixed_batch(9, 8, 1, seed=65)
    ids = np.zeros(9, dtype=np.int32)
    want = single_float_plan(cfg[0]).synthesize_host(params, frames)
    vp = float_voices_plan(cfg)
    assert vp.n_voices == 1
    for got in (vp.synthesize_host(params, ids, frames), g.Plan.synthesize_host(vp, params, frames)):
        for w, x in zip(want, got):
            assert np.array_equal(w, x)
    # its streams, too: gvtm_stream_create_voices and gvtm_stream_create
    for st in (g.Stream(vp, 9, voice_ids=ids), g.Stream(vp, 9)):
        pieces = st.push(params, frames)
        tails, peak = st.finish()
        for b in range(9):
            assert np.array_equal(np.concatenate([pieces[b], tails[b]]), want[0][b, : want[1][b]]) and peak[b] == want[2][b], b


# ---- 6. out-of-range voice ids -----------------------------------------------------------------------------------------------

def test_out_of_range_voice_ids_fail_alone():
    plan = plan_of()
    params, ids, frames = mixed_batch(24, 10, 5, seed=66)
    bad = ids.copy()
    bad[[3, 10, 17]] = [-1, 5, 1 << 20]
    stride = plan.voices_output_capacity(10)
    good_audio, good_counts, good_max = run_voices_device(plan, params, ids, frames, stride)
    audio, counts, maxabs = run_voices_device(plan, params, bad, frames, stride, fill=7.0)
    for b in range(24):
        if b in (3, 10, 17):
            assert counts[b] == -1 and maxabs[b] == 0.0
            assert (audio[b] == 7.0).all()  # the device entry leaves the row untouched
        else:
            n = int(good_counts[b])
            assert counts[b] == n and maxabs[b] == good_max[b]
            assert np.array_equal(audio[b, :n], good_audio[b, :n]) and (audio[b, n:] == 7.0).all()
    h_audio, h_counts, h_max = plan.synthesize_host(params, bad, frames)
    assert (h_counts[[3, 10, 17]] == -1).all() and not h_audio[[3, 10, 17]].any() and not h_max[[3, 10, 17]].any()
    for b in set(range(24)) - {3, 10, 17}:
        n = int(good_counts[b])
        assert h_counts[b] == n and h_max[b] == good_max[b] and np.array_equal(h_audio[b, :n], good_audio[b, :n]), b


# ---- 7. the host entries slice a big mixed batch -------------------------------------------------------------------------------

def test_host_entries_slice_a_big_mixed_batch():
    """Two machine-fulls and more of the chunk-56 shape (two utterances per compute unit): the host pipeline cuts the
    batch into slices, each with its own grouping; float and pcm16 host entries against the device entry in one launch."""
    import torch
    plan = plan_of()
    batch, max_frames = 4 * torch.cuda.get_device_properties(0).multi_processor_count + 77, 5
    params, ids, frames = mixed_batch(batch, max_frames, 5, seed=67)
    stride = plan.voices_output_capacity(max_frames)
    d_audio, d_counts, d_max = run_voices_device(plan, params, ids, frames, stride)
    for b in range(batch):
        assert d_counts[b] == plan.voice_output_count(int(ids[b]), int(frames[b]))
    audio, counts, maxabs = plan.synthesize_host(params, ids, frames)
    assert np.array_equal(counts, d_counts) and np.array_equal(maxabs, d_max)
    for b in range(batch):
        n = int(counts[b])
        assert np.array_equal(audio[b, :n], d_audio[b, :n]) and not audio[b, n:].any(), b
        assert maxabs[b] == (np.abs(audio[b, :n]).max() if n else 0.0)
    pcm, p_counts, p_max, scales = plan.synthesize_host_pcm16(params, ids, frames)
    assert np.array_equal(p_counts, d_counts) and np.array_equal(p_max, d_max)
    da = torch.from_numpy(np.ascontiguousarray(np.where(np.arange(stride)[None, :] < d_counts[:, None], d_audio, 0.0).astype(np.float32))).cuda()
    di16 = torch.zeros((batch, stride), dtype=torch.int16, device="cuda")
    ds = torch.zeros(batch, dtype=torch.float32, device="cuda")
    plan.normalize_device(da, batch, stride, torch.from_numpy(d_max).cuda(), torch.from_numpy(d_counts).cuda(), None, di16, ds,
                          torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(pcm, di16.cpu().numpy()) and np.array_equal(scales, ds.cpu().numpy())


# ---- 8. streams ------------------------------------------------------------------------------------------------------------------

def push_in_pieces(st, params, total, pieces):
    """total[b] frames of utterance b pushed in pieces of at most pieces[i] frames, then finished -> (samples, maxabs)."""
    total = np.asarray(total, dtype=np.int32)
    outs = [[] for _ in total]
    done = np.zeros(len(total), dtype=np.int32)
    for n in pieces:
        fc = np.minimum(n, total - done).astype(np.int32)
        buf = np.zeros((len(total), n, 16), np.float32)
        for b in range(len(total)):
            buf[b, : fc[b]] = params[b, done[b]: done[b] + fc[b]]
        for b, piece in enumerate(st.push(buf, fc)):
            outs[b].append(piece)
        done += fc
    assert (done == total).all()
    tails, maxabs = st.finish()
    return [np.concatenate(outs[b] + [tails[b]]) for b in range(len(total))], maxabs


STREAM_IDS = np.array([0, 3, 1, 4, 2, 3, 0, 2, 4, 1], dtype=np.int32)
RAGGED_TOTAL = np.array([33, 20, 8, 33, 1, 29, 0, 17, 5, 26], dtype=np.int32)
LOCKSTEP_TOTAL = np.array([30, 21, 33, 26, 28], dtype=np.int32)[STREAM_IDS]  # within a voice, every utterance moves alike


@SHAPES
@pytest.mark.parametrize("total", [RAGGED_TOTAL, LOCKSTEP_TOTAL], ids=["ragged", "lockstep_per_voice"])
def test_stream_pieces_equal_the_one_shot_launch_and_the_oracle(total, rows):
    plan = plan_of(rows=rows)
    params = tracks.random_tracks(len(STREAM_IDS), 33, seed0=6800, consonant_heavy=True)
    one, c1, m1 = plan.synthesize_host(params, STREAM_IDS, total)
    got, maxabs = push_in_pieces(g.Stream(plan, len(STREAM_IDS), voice_ids=STREAM_IDS), params, total, (7, 1, 25))
    for b, v in enumerate(STREAM_IDS):
        assert got[b].size == c1[b] == plan.voice_output_count(int(v), int(total[b])), b
        assert within(got[b], one[b, : c1[b]], BIT_IDENTICAL) and maxabs[b] == m1[b], b
        ref = shared(("stream", int(total[b]), b), lambda: oracle_ref(VOICES[v], cases.RATE, params[b, : total[b]]))
        assert got[b].size == ref.size and within(got[b], ref, BIT_IDENTICAL), b
        assert maxabs[b] == (np.abs(ref).max() if ref.size else 0.0), b


@SHAPES
def test_stream_finish_on_a_flush_overrun_of_female_in_a_mixed_stream(rows, golden):
    """167 frames of female at 44.1 kHz next to the other voices: finish converts the extra lap of the ring, and the
    samples are the real class's (female_ovr_5f)."""
    case = cases.by_name("female_ovr_5f")
    f, rate = cases.OVERRUN_FRAMES["female"], cases.OVERRUN_RATE["female"]
    assert case["rate"] == rate and case["track"][1] == f
    plan = plan_of(rate, rows)
    ids = np.array([2, 1, 0, 4, 3], dtype=np.int32)
    total = np.array([9, f, 12, 3, 6], dtype=np.int32)
    params = tracks.random_tracks(5, f, seed0=6900, consonant_heavy=True)
    params[1] = cases.track_for(case, golden)
    got, maxabs = push_in_pieces(g.Stream(plan, 5, voice_ids=ids), params, total, (7, 1, 25, 134))
    assert got[1].size == plan.voice_output_count(1, f) > plan.voice_output_count(1, f + 1)
    check_vector(case, got[1], got[1].size, maxabs[1], golden)
    one, c1, m1 = plan.synthesize_host(params, ids, total)
    for b in range(5):
        assert got[b].size == c1[b] and within(got[b], one[b, : c1[b]], BIT_IDENTICAL) and maxabs[b] == m1[b], b


def test_reset_voices_gives_the_permuted_voices_samples():
    plan = plan_of()
    params = tracks.random_tracks(len(STREAM_IDS), 33, seed0=6800, consonant_heavy=True)
    st = g.Stream(plan, len(STREAM_IDS), voice_ids=STREAM_IDS)
    first, first_max = push_in_pieces(st, params, RAGGED_TOTAL, (7, 1, 25))
    perm = np.array([4, 0, 2, 1, 3, 3, 1, 0, 2, 4], dtype=np.int32)
    st.reset(perm)
    moved, moved_max = push_in_pieces(st, params, RAGGED_TOTAL, (7, 1, 25))
    singles = singles_of(configs5f(), params, perm, RAGGED_TOTAL)
    for b in range(len(perm)):
        ref, n, peak = singles[b]
        assert moved[b].size == n and within(moved[b], ref, BIT_IDENTICAL) and moved_max[b] == peak, b
    assert moved[0].size != first[0].size or not np.array_equal(moved[0], first[0])  # voice 4 now, not voice 0
    # reset() keeps the ids
    st.reset()
    again, again_max = push_in_pieces(st, params, RAGGED_TOTAL, (7, 1, 25))
    for b in range(len(perm)):
        assert np.array_equal(again[b], moved[b]) and again_max[b] == moved_max[b], b


# ---- 9. event lists --------------------------------------------------------------------------------------------------------------

def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_events_voices_entry_equals_the_single_voice_float_events_entry():
    """Event lists of a mix of voices in, samples out: frame counts, samples, counts, peaks and drift states bit for bit as
    gvtm_synthesize_events_device gives them on the single-voice float plan of each voice with that voice's track
    configuration."""
    cfgs = configs5f()
    tcs = track_configs(model5=True)
    plan = float_voices_plan(cfgs)
    plan.set_voice_tracks(tcs)
    batch = 15
    pool = [singable_event_table(seed, n) for seed, n in SINGABLE]
    tables = [pool[(7 * b) % len(pool)] for b in range(batch)]
    ids = np.array([b % 5 for b in range(batch)], dtype=np.int32)
    frames_of = [capi.tracks_frame_count(tcs[v], capi.events_from_table(t)) for t, v in zip(tables, ids)]
    max_frames = max(frames_of)
    assert all(max(frames_of[b] for b in range(batch) if ids[b] == v) > 0 for v in range(5))
    stride = plan.voices_output_capacity(max_frames)
    drift0 = fresh_drift(batch)
    got = synthesize_events(plan, tables, max_frames, stride, drift0, ids=ids)
    for v in range(5):
        sel = np.nonzero(ids == v)[0]
        idx = np.concatenate([sel, np.zeros(batch - sel.size, dtype=np.intp)])  # (filler lists keep the batch size)
        single = single_float_plan(cfgs[v])
        one = synthesize_events(single, [tables[i] for i in idx], max_frames, single.output_capacity(max_frames), drift0[idx], track_config=tcs[v])
        for j, b in enumerate(sel):
            assert got["frames"][b] == one["frames"][j] == frames_of[b], b
            n = int(one["counts"][j])
            assert np.isfinite(one["audio"][j]).all() and np.isfinite(one["maxabs"][j]), b
            assert got["counts"][b] == n == plan.voice_output_count(v, frames_of[b]) <= stride, b
            assert same_bits(got["audio"][b, :n], one["audio"][j, :n]) and not got["audio"][b, n:].any(), b
            assert same_bits(got["maxabs"][b], one["maxabs"][j]) and got["maxabs"][b] == (np.abs(got["audio"][b, :n]).max() if n else 0.0), b
            assert same_bits(got["drift"][b], one["drift"][j]), b
