"""Event lists of a batch that mixes voices (gvtm_plan_set_voice_tracks, gvtm_generate_tracks_voices_device,
gvtm_synthesize_events_voices_device).

Track generation depends on the voice (mean pitch = pitch offset + the variant's reference_glottal_pitch, initial pitch,
intonation flags, drift set-up: Controller.cpp:70-81), so the tracks kernel picks its constants per utterance.  Every
utterance's frames, frame count and drift state must be bit for bit what the single-configuration kernel and the tracks
oracle give under its voice's configuration, and its samples bit for bit those of gvtm_synthesize_events_device on a
single-voice plan of its voice."""
import numpy as np
import pytest

import gama_tts_amd as g
from gama_tts_amd import capi
import event_lists
import model5_cases as cases5
import oracle
from device_io import events_on_device, generate_tracks, synthesize_events
from parity_rules import TOL, check_model5, within
from track_cases import fresh_drift, product_config, singable_event_table, used_drift
from voice_cases import configs, configs5, mixed_batch, oracle_config
from voice_files import VOICES

pytestmark = pytest.mark.gpu

# the ten numbers of a track configuration (oracle.track_config): control period, macro, micro, drift, smooth, initial pitch,
# mean pitch, drift deviation / sample rate / cutoff
# the five variants of 0_male: its vtm_control_model.txt, mean pitch = -4 + reference_glottal_pitch
VARIANT_TRACKS = [np.array([4, 1, 1, 1, 1, -20.0, mean, 4.0, 250.0, 4.0]) for mean in (-16.0, -4.0, -1.5, 1.0, 3.5)]
# five configurations that differ in everything a voice may: one each with drift, macro, micro and smooth intonation off
DIVERSE_TRACKS = [np.array([4, 1, 1, 1, 1, -20.0, -16.0, 4.0, 250.0, 4.0]),
                  np.array([4, 1, 1, 0, 1, -18.0, -4.0, 3.0, 250.0, 4.0]),
                  np.array([4, 0, 1, 1, 1, -20.0, -1.5, 5.0, 250.0, 6.0]),
                  np.array([4, 1, 0, 1, 1, -22.5, 1.0, 2.0, 250.0, 3.0]),
                  np.array([4, 1, 1, 1, 0, -15.0, 3.5, 4.0, 200.0, 4.0])]
# the (seed, events) pairs of test_gpu_tracks' pool that every voice and model can sing (fresh drift generators; 44.1 kHz at
# SectionDelay 1 and 2, double and float; model 5 at 48 kHz): with these, every list that yields frames stays finite
SINGABLE = [(300, 40), (301, 2), (302, 1), (303, 17), (305, 3), (306, 55), (307, 9), (308, 33), (309, 25)]


def frame_counts_of(cfgvs, tables, ids):
    return [capi.tracks_frame_count(product_config(cfgvs[v]), capi.events_from_table(t)) if 0 <= v < len(cfgvs) else 0
            for t, v in zip(tables, ids)]


def voices_plan(cfgs, cfgvs):
    plan = g.VoicesPlan(cfgs, 250.0, 0)
    plan.set_voice_tracks([product_config(c) for c in cfgvs])
    return plan


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- 1. frames, bit for bit

def test_frames_counts_and_drift_states_are_those_of_each_voices_configuration():
    lengths = [40, 2, 1, 17, 80, 3, 55, 9, 33, 110, 111, 150, 260, 239, 240, 241]  # (tabled up to 240 events; 241 and 260 walk memory)
    tables = [event_lists.random_event_table(100 + b, n_events=n) for b, n in enumerate(lengths)]
    ids = [b % 5 for b in range(len(tables))]
    bad = 6
    tables.insert(bad, event_lists.random_event_table(99, n_events=40))
    ids.insert(bad, 7)
    batch = len(tables)
    assert batch % 2 == 1  # the last workgroup holds one utterance
    assert sorted(set(ids) - {7}) == [0, 1, 2, 3, 4] and all(ids[b] != ids[b + 1] for b in range(batch - 1))
    drift0 = used_drift(batch)
    want = [oracle.tracks_generate(oracle.track_config(DIVERSE_TRACKS[v]), t, tuple(drift0[b])) if v < 5 else None
            for b, (t, v) in enumerate(zip(tables, ids))]
    max_frames = max(w[0].shape[0] for w in want if w)
    plan = voices_plan(configs(precision=capi.PRECISION_F32), DIVERSE_TRACKS)
    params, counts, drift = generate_tracks(tables, max_frames, drift0, plan=plan, ids=ids)
    singles = [generate_tracks(tables, max_frames, drift0, track_config=product_config(c)) for c in DIVERSE_TRACKS]
    for b, v in enumerate(ids):
        if b == bad:
            assert counts[b] == 0
            assert (params[b] == 7.0).all() and same_bits(drift[b], drift0[b])
            continue
        frames, state = want[b]
        n = frames.shape[0]
        assert counts[b] == n, (b, v)
        assert np.array_equal(params[b, :n].view(np.uint32), frames.view(np.uint32)), (b, v)
        assert (params[b, n:] == 7.0).all()
        assert tuple(drift[b]) == state, (b, v)
        s_params, s_counts, s_drift = singles[v]
        assert s_counts[b] == n
        assert np.array_equal(params[b, :n].view(np.uint32), s_params[b, :n].view(np.uint32)), (b, v)
        assert same_bits(drift[b], s_drift[b]), (b, v)
    # the voices differ: the same list under two configurations does not give the same frames
    assert not np.array_equal(singles[0][0][0], singles[1][0][0])
    # rows shorter than the longest list: cut there, the counts and the drift states still those of the whole lists
    cut = max_frames - 37
    assert sum(1 for w in want if w and w[0].shape[0] > cut) >= 1 and cut > 0
    params2, counts2, drift2 = generate_tracks(tables, cut, drift0, plan=plan, ids=ids)
    assert np.array_equal(counts2, counts) and same_bits(drift2, drift)
    for b in range(batch):
        if b == bad:
            assert (params2[b] == 7.0).all()
            continue
        n = min(int(counts[b]), cut)
        assert np.array_equal(params2[b, :n].view(np.uint32), params[b, :n].view(np.uint32)), b
        assert (params2[b, n:] == 7.0).all()


# ---- 2. pinned to the reference directly

def test_captured_reference_calls_next_to_other_voices(golden_tracks):
    cfg_hello, _, _ = event_lists.load_golden(golden_tracks, "hello", 0)
    cfgvs = []
    for v, shift in enumerate([-12.0, -3.0, 0.0, 2.5, 7.0]):  # voice 2: the captured configuration; the rest: other mean pitches
        c = np.array(cfg_hello, dtype=np.float64)
        c[6] += shift
        cfgvs.append(c)
    plan = voices_plan(configs(precision=capi.PRECISION_F32), cfgvs)
    captured = [event_lists.load_golden(golden_tracks, name, 0) for name in event_lists.CAPTURED]
    tables, ids = [], []
    for q, (_, events, _) in enumerate(captured):  # each text under voice 2 and, next to it, under one of the others
        tables += [events, events]
        ids += [2, [0, 1, 3, 4][q]]
    batch = len(tables)
    max_frames = max(c[2].shape[0] for c in captured) + 3
    params, counts, drift = generate_tracks(tables, max_frames, fresh_drift(batch), plan=plan, ids=ids)
    for q, (cfg, events, frames) in enumerate(captured):
        n = frames.shape[0]
        assert counts[2 * q] == n and counts[2 * q + 1] == n
        assert np.array_equal(params[2 * q, :n].view(np.uint32), frames.view(np.uint32)), event_lists.CAPTURED[q]
        other, state = oracle.tracks_generate(oracle.track_config(cfgvs[ids[2 * q + 1]]), events)
        assert np.array_equal(params[2 * q + 1, :n].view(np.uint32), other.view(np.uint32)), event_lists.CAPTURED[q]
        assert tuple(drift[2 * q + 1]) == state
        assert not np.array_equal(params[2 * q + 1, :n, 0], params[2 * q, :n, 0])  # another mean pitch


# ---- 3. audio equals the single-voice events entry

def singable_batch(batch):
    pool = [singable_event_table(seed, n) for seed, n in SINGABLE]
    tables = [pool[(7 * b) % len(pool)] for b in range(batch)]  # (the first five: 40, 33, 55, 17 and 2 events)
    ids = np.array([b % 5 for b in range(batch)], dtype=np.int32)
    return tables, ids


def singles_of_events(make_plan, cfgvs, tables, ids, max_frames, drift0):
    """Every utterance through gvtm_synthesize_events_device on a single-voice plan of its voice, with its voice's track
    configuration: the same batch size (filler lists keep the workgroup shape), that voice's rows kept.
    -> {b: dict of that utterance's outputs}"""
    out = {}
    for v in range(len(cfgvs)):
        sel = np.nonzero(np.asarray(ids) == v)[0]
        if sel.size == 0:
            continue
        idx = np.concatenate([sel, np.zeros(len(ids) - sel.size, dtype=np.intp)])
        plan = make_plan(v)
        r = synthesize_events(plan, [tables[i] for i in idx], max_frames, plan.output_capacity(max_frames), drift0[idx],
                              track_config=product_config(cfgvs[v]))
        for j, b in enumerate(sel):
            out[int(b)] = {k: a[j] for k, a in r.items()}
    return out


def assert_as_singles(got, singles, ids, frames_of, stride):
    for b in range(len(ids)):
        one = singles[b]
        if frames_of[b] > 0:  # every list that yields frames is singable: compared without exception
            assert np.isfinite(one["audio"]).all() and np.isfinite(one["maxabs"]), b
        assert got["frames"][b] == one["frames"] == frames_of[b], b
        n = int(one["counts"])
        assert got["counts"][b] == n and n <= stride, b
        assert same_bits(got["audio"][b, :n], one["audio"][:n]), (b, int(ids[b]))
        assert not got["audio"][b, n:].any()
        assert same_bits(got["maxabs"][b], one["maxabs"]), b
        assert same_bits(got["drift"][b], one["drift"]), b


EVENTS_CASES = [(batch, precision, delay) for batch in (5, 300, 601) for precision in (capi.PRECISION_F32, capi.PRECISION_F64, capi.PRECISION_MIXED)
                for delay in (1, 2) if not (batch > 5 and delay == 2 and precision == capi.PRECISION_MIXED)]  # (covered by the others)
ROWS = {5: "one_row", 300: "two_rows", 601: "four_rows"}
PRECISIONS = {capi.PRECISION_F32: "f32", capi.PRECISION_F64: "f64", capi.PRECISION_MIXED: "mixed"}


@pytest.mark.parametrize("batch,precision,delay", EVENTS_CASES, ids=["%s-%s-d%d" % (ROWS[b], PRECISIONS[p], d) for b, p, d in EVENTS_CASES])
def test_events_voices_entry_equals_the_single_voice_events_entry(batch, precision, delay):
    cfgs = configs(44100.0, delay, precision)
    plan = voices_plan(cfgs, VARIANT_TRACKS)
    tables, ids = singable_batch(batch)
    frames_of = frame_counts_of(VARIANT_TRACKS, tables, ids)
    max_frames = max(frames_of)
    stride = plan.voices_output_capacity(max_frames)
    drift0 = fresh_drift(batch)
    got = synthesize_events(plan, tables, max_frames, stride, drift0, ids=ids)
    singles = singles_of_events(lambda v: g.Plan(cfgs[v], 250.0, 0), VARIANT_TRACKS, tables, ids, max_frames, drift0)
    assert_as_singles(got, singles, ids, frames_of, stride)
    # one utterance per voice through the oracles: the tracks oracle's frames, then the vocal-tract oracle of that voice
    for v, name in enumerate(VOICES):
        b = max((b for b in range(batch) if ids[b] == v), key=lambda b: frames_of[b])
        frames, _ = oracle.tracks_generate(oracle.track_config(VARIANT_TRACKS[v]), tables[b])
        assert frames.shape[0] == frames_of[b] > 0
        ref = oracle.synthesize(oracle_config(name, 44100.0, delay, 0, precision), frames)
        assert got["counts"][b] == ref.size and np.isfinite(ref).all()
        assert within(got["audio"][b, : ref.size], ref, TOL[precision]), (b, name)


def test_events_voices_entry_on_a_model5_plan():
    cfgs = configs5(48000.0)
    plan = voices_plan(cfgs, VARIANT_TRACKS)
    batch = 15
    tables, ids = singable_batch(batch)
    frames_of = frame_counts_of(VARIANT_TRACKS, tables, ids)
    max_frames = max(frames_of)
    stride = plan.voices_output_capacity(max_frames)
    drift0 = fresh_drift(batch)
    got = synthesize_events(plan, tables, max_frames, stride, drift0, ids=ids)
    singles = singles_of_events(lambda v: g.Plan(cfgs[v], 250.0, 0), VARIANT_TRACKS, tables, ids, max_frames, drift0)
    assert_as_singles(got, singles, ids, frames_of, stride)
    for v, name in enumerate(VOICES):
        b = max((b for b in range(batch) if ids[b] == v), key=lambda b: frames_of[b])
        frames, _ = oracle.tracks_generate(oracle.track_config(VARIANT_TRACKS[v]), tables[b])
        ref, _ = oracle.synthesize5(cases5.voice_oracle_config(name, 48000.0), frames)
        assert got["counts"][b] == ref.size and np.isfinite(ref).all()
        check_model5(got["audio"][b, : ref.size], ref)


# ---- 4. a one-voice plan

@pytest.mark.parametrize("precision", [capi.PRECISION_F32, capi.PRECISION_F64], ids=["f32", "f64"])
def test_one_voice_plan_equals_the_events_entry(precision):
    cfg = configs(precision=precision, names=["female"])
    cfgv = DIVERSE_TRACKS[3]
    plan = voices_plan(cfg, [cfgv])
    batch = 45
    tables, _ = singable_batch(batch)
    max_frames = max(frame_counts_of([cfgv], tables, [0] * batch))
    stride = plan.voices_output_capacity(max_frames)
    drift0 = fresh_drift(batch)
    got = synthesize_events(plan, tables, max_frames, stride, drift0, ids=np.zeros(batch, dtype=np.int32))
    want = synthesize_events(g.Plan(cfg[0], 250.0, 0), tables, max_frames, stride, drift0, track_config=product_config(cfgv))
    assert (want["frames"] > 0).sum() >= batch // 2
    for k in want:
        assert same_bits(got[k], want[k]), k


# ---- 5. bad ids in the synthesis entry

def test_out_of_range_voice_ids_fail_alone():
    plan = voices_plan(configs(precision=capi.PRECISION_F32), VARIANT_TRACKS)
    tables, ids = singable_batch(24)
    bad_at = {3: -1, 10: 5}
    bad = ids.copy()
    for b, v in bad_at.items():
        bad[b] = v
    keep = [b for b in range(24) if b not in bad_at]
    frames_of = frame_counts_of(VARIANT_TRACKS, tables, ids)
    max_frames = max(frames_of)
    stride = plan.voices_output_capacity(max_frames)
    drift0 = fresh_drift(24)
    got = synthesize_events(plan, tables, max_frames, stride, drift0, ids=bad, fill=7.0)
    good = synthesize_events(plan, [tables[b] for b in keep], max_frames, stride, drift0[keep], ids=ids[keep], fill=7.0)
    for b in bad_at:
        assert got["counts"][b] == -1 and got["maxabs"][b] == 0.0 and got["frames"][b] == 0
        assert (got["audio"][b] == 7.0).all() and same_bits(got["drift"][b], drift0[b])
    for k in good:
        assert same_bits(got[k][keep], good[k]), k
    assert (good["counts"] >= 0).all() and (good["frames"] == np.array(frames_of)[keep]).all()


# ---- 6. enqueue-only holds

@pytest.mark.parametrize("precision", [capi.PRECISION_F32, capi.PRECISION_F64], ids=["f32", "f64"])
def test_events_voices_entry_keeps_its_buffers_while_a_host_entry_runs(precision):
    """gvtm_synthesize_events_voices_device only enqueues.  The voices host entry called on the same plan while its kernels
    are still queued (other utterances, more frames each: it grows its own staging, grouping and the noise-sample table)
    must leave the events-voices entry's frames, grouping and tables alone: both calls come out bit for bit as each does
    alone."""
    import torch
    plan = voices_plan(configs(precision=precision), VARIANT_TRACKS)
    pool = [singable_event_table(700 + b, n) for b, n in enumerate([40, 25, 60, 33])]
    batch = 4096  # some milliseconds of synthesis: the host entry is called long before it is done
    tables = [pool[b % len(pool)] for b in range(batch)]
    ids = np.array([(b // 4 + b) % 5 for b in range(batch)], dtype=np.int32)
    max_frames = max(capi.tracks_frame_count(product_config(VARIANT_TRACKS[0]), capi.events_from_table(t)) for t in pool)
    stride = plan.voices_output_capacity(max_frames)
    h_params, h_ids, h_frames = mixed_batch(64, 2 * max_frames, 5, seed=92)
    d_events, d_offsets = events_on_device(tables)
    dev = d_events.device
    d_ids = torch.from_numpy(ids).to(dev)
    side = torch.cuda.Stream()  # a non-blocking stream: nothing orders it against the host entry's own streams

    def enqueue_events():
        a = torch.zeros((batch, stride), dtype=torch.float32, device=dev)
        f = torch.zeros(batch, dtype=torch.int32, device=dev)
        n = torch.zeros(batch, dtype=torch.int64, device=dev)
        m = torch.zeros(batch, dtype=torch.float32, device=dev)
        side.wait_stream(torch.cuda.current_stream())
        plan.synthesize_events_voices_device(d_events, d_offsets, d_ids, batch, max_frames, a, stride, f, n, m, None, side.cuda_stream)
        return a, f, n, m

    both = enqueue_events()
    host_both = plan.synthesize_host(h_params, h_ids, h_frames)  # no synchronisation in between
    torch.cuda.synchronize()
    alone = enqueue_events()
    torch.cuda.synchronize()
    host_alone = plan.synthesize_host(h_params, h_ids, h_frames)
    assert int((both[2] > 0).sum().item()) == batch
    for x, y in zip(both, alone):  # samples, frame counts, sample counts, peaks: bit for bit
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    for x, y in zip(host_both, host_alone):
        assert x.tobytes() == y.tobytes()
