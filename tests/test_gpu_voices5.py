"""Several reference model 5 voices in one batched launch (gvtm_plan_create_model5_voices + gvtm_synthesize_voices_*).

The five variants of data/voice/english/5_male (tests/golden/voice5_*.txt: vocal tract 17.5 / 15 / 12.5 / 10 / 7.5 cm,
242 to 564 internal steps per frame) mixed in one batch, ids interleaved and ragged.  Every utterance must come out bit for
bit as a single-voice model 5 plan of its voice synthesizes it, and within model 5's bar (parity_rules.check_model5) of the oracle and of
the reference vectors of tests/golden/voices5_golden.npz."""
import numpy as np
import pytest

import gama_tts_amd as g
import model5_cases as cases
import oracle
import voice_files
from device_io import run_voices_device
from parity_rules import check_model5
from voice_cases import configs5, mixed_batch, padded

pytestmark = pytest.mark.gpu

CASES = cases.CASES["voices5"]


def singles_of(cfgs, params, ids, frames):
    """Every utterance through a single-voice model 5 plan of its voice: {b: (samples, count, maxabs)}."""
    out = {}
    for v, cfg in enumerate(cfgs):
        sel = np.nonzero(ids == v)[0]
        if sel.size == 0:
            continue
        audio, counts, maxabs = g.Plan(cfg, 250.0, 0).synthesize_host(params[sel], frames[sel])
        for j, b in enumerate(sel):
            out[int(b)] = (audio[j, : counts[j]], int(counts[j]), float(maxabs[j]))
    return out


def assert_as_singles(audio, counts, maxabs, singles, ids):
    for b in range(len(ids)):
        ref, n, peak = singles[b]
        assert counts[b] == n, b
        assert np.array_equal(audio[b, :n], ref), (b, int(ids[b]))
        assert maxabs[b] == peak, b


@pytest.fixture(scope="module")
def plan5():
    return g.VoicesPlan(configs5(), 250.0, 0)


def test_five_voices_in_one_launch(plan5):
    cfgs = configs5()
    assert plan5.n_voices == 5 and all(plan5.voice_info(v).model5 == 1 for v in range(5))
    params, ids, frames = mixed_batch(45, 14, 5, seed=51)
    stride = plan5.voices_output_capacity(14)
    audio, counts, maxabs = run_voices_device(plan5, params, ids, frames, stride)
    for b in range(len(ids)):
        assert counts[b] == plan5.voice_output_count(int(ids[b]), int(frames[b]))
    assert_as_singles(audio, counts, maxabs, singles_of(cfgs, params, ids, frames), ids)
    # the two longest utterances of every voice against the oracle
    for v, name in enumerate(voice_files.VOICES):
        sel = np.nonzero(ids == v)[0]
        for b in sel[np.argsort(frames[sel])[-2:]]:
            ref, _ = oracle.synthesize5(cases.voice_oracle_config(name), params[b, : frames[b]])
            assert counts[b] == ref.size
            check_model5(audio[b, : ref.size], ref)


def test_diagnostics_two_row_shape_gives_one_row_to_voices(plan5):
    # a plan that forces two utterances per workgroup runs its voices launches with one (the voice variant's only shape)
    params, ids, frames = mixed_batch(20, 8, 5, seed=52)
    stride = plan5.voices_output_capacity(8)
    want = run_voices_device(plan5, params, ids, frames, stride)
    diag = g.VoicesPlan(configs5(), 250.0, 0, diagnostics=True, rows=2)
    got = run_voices_device(diag, params, ids, frames, stride)
    for w, x in zip(want, got):
        assert np.array_equal(w, x)


@pytest.mark.parametrize("rate", sorted({c["rate"] for c in CASES}), ids=lambda r: "%dHz" % r)
def test_reference_vectors_through_a_mixed_launch(rate, golden):
    """The reference's own output for the four new voices, every case of this output rate in one mixed launch (a male
    utterance in between)."""
    golden5v = cases.load("voices5")
    sel = [c for c in CASES if c["rate"] == rate]
    trs = [cases.track_for(c, golden) for c in sel]
    male = cases.track_for(dict(track=("random", 60, 70, True)))
    trs.append(male)
    ids = np.array([voice_files.VOICES.index(c["voice"]) for c in sel] + [0], dtype=np.int32)
    params, frames = padded(trs)
    plan = g.VoicesPlan(configs5(rate), 250.0, 0)
    audio, counts, maxabs = plan.synthesize_host(params, ids, frames)
    for b, c in enumerate(sel):
        m = golden5v["manifest"][c["name"]]
        assert abs(plan.voice_info(int(ids[b])).internal_rate_hz - m["fs"]) < 1e-6
        assert counts[b] == m["n"], c["name"]
        for got, key in cases.stored(c, audio[b, : m["n"]]):
            check_model5(got, golden5v[key], peak=m["maxabs"])
        assert maxabs[b] == pytest.approx(m["maxabs"], rel=1e-5)
    ref, _ = oracle.synthesize5(cases.voice_oracle_config("male", rate), male)
    assert counts[-1] == ref.size
    check_model5(audio[-1, : ref.size], ref)


def test_out_of_range_voice_ids_fail_alone(plan5):
    params, ids, frames = mixed_batch(24, 10, 5, seed=53)
    bad = ids.copy()
    bad[[3, 10, 17]] = [-1, 5, 1 << 20]
    stride = plan5.voices_output_capacity(10)
    good_audio, good_counts, good_max = run_voices_device(plan5, params, ids, frames, stride)
    audio, counts, maxabs = run_voices_device(plan5, params, bad, frames, stride, fill=7.0)
    for b in range(24):
        if b in (3, 10, 17):
            assert counts[b] == -1 and maxabs[b] == 0.0
            assert (audio[b] == 7.0).all()  # the device entry leaves the row untouched
        else:
            n = int(good_counts[b])
            assert counts[b] == n and maxabs[b] == good_max[b]
            assert np.array_equal(audio[b, :n], good_audio[b, :n])
    h_audio, h_counts, h_max = plan5.synthesize_host(params, bad, frames)
    assert (h_counts[[3, 10, 17]] == -1).all() and not h_audio[[3, 10, 17]].any() and not h_max[[3, 10, 17]].any()


def test_a_batch_of_one_voice_only(plan5):
    params, _, frames = mixed_batch(20, 10, 5, seed=54)
    ids = np.full(20, 4, dtype=np.int32)  # baby: 564 steps per frame
    audio, counts, maxabs = run_voices_device(plan5, params, ids, frames, plan5.voices_output_capacity(10))
    assert_as_singles(audio, counts, maxabs, singles_of(configs5(), params, ids, frames), ids)


def test_more_workgroups_than_compute_units(plan5):
    # 600 utterances: more than one workgroup per compute unit, and a padding workgroup per voice past the last one
    params, ids, frames = mixed_batch(600, 6, 5, seed=55)
    audio, counts, maxabs = run_voices_device(plan5, params, ids, frames, plan5.voices_output_capacity(6))
    assert_as_singles(audio, counts, maxabs, singles_of(configs5(), params, ids, frames), ids)


def test_host_entries_slice_a_big_mixed_batch(plan5):
    """Two machine-fulls and more (one utterance per workgroup x the compute units): the host pipeline cuts the batch
    into slices, each with its own grouping; float and pcm16 host entries against the device entry in one launch."""
    import torch
    batch, max_frames = 2 * torch.cuda.get_device_properties(0).multi_processor_count + 77, 5
    params, ids, frames = mixed_batch(batch, max_frames, 5, seed=56)
    stride = plan5.voices_output_capacity(max_frames)
    d_audio, d_counts, d_max = run_voices_device(plan5, params, ids, frames, stride)
    audio, counts, maxabs = plan5.synthesize_host(params, ids, frames)
    assert np.array_equal(counts, d_counts) and np.array_equal(maxabs, d_max)
    for b in range(batch):
        n = int(counts[b])
        assert np.array_equal(audio[b, :n], d_audio[b, :n]) and not audio[b, n:].any(), b
    pcm, p_counts, p_max, scales = plan5.synthesize_host_pcm16(params, ids, frames)
    assert np.array_equal(p_counts, d_counts) and np.array_equal(p_max, d_max)
    da = torch.from_numpy(np.ascontiguousarray(np.where(np.arange(stride)[None, :] < d_counts[:, None], d_audio, 0.0).astype(np.float32))).cuda()
    di16 = torch.zeros((batch, stride), dtype=torch.int16, device="cuda")
    ds = torch.zeros(batch, dtype=torch.float32, device="cuda")
    plan5.normalize_device(da, batch, stride, torch.from_numpy(d_max).cuda(), torch.from_numpy(d_counts).cuda(), None, di16, ds,
                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(pcm, di16.cpu().numpy()) and np.array_equal(scales, ds.cpu().numpy())


def test_one_voice_model5_plan_takes_the_voices_entries():
    cfg = configs5(names=["small_child"])
    params, _, frames = mixed_batch(9, 8, 1, seed=57)
    ids = np.zeros(9, dtype=np.int32)
    single = g.Plan(cfg[0], 250.0, 0)
    want = single.synthesize_host(params, frames)
    # a gvtm_plan_create_model5 plan through gvtm_synthesize_voices_host
    stride = single.output_capacity(8)
    audio = np.zeros((9, stride), dtype=np.float32)
    counts = np.zeros(9, dtype=np.int64)
    maxabs = np.zeros(9, dtype=np.float32)
    p = np.ascontiguousarray(params)
    f = np.ascontiguousarray(frames)
    single._check(single._lib.gvtm_synthesize_voices_host(single._h, p.ctypes.data, f.ctypes.data, ids.ctypes.data, 8, 9,
                                                          audio.ctypes.data, stride, counts.ctypes.data, maxabs.ctypes.data))
    assert np.array_equal(counts, want[1]) and np.array_equal(maxabs, want[2])
    assert np.array_equal(audio, want[0][:, :stride])
    # a one-voice gvtm_plan_create_model5_voices plan: its voices entries and its batch entries
    vp = g.VoicesPlan(cfg, 250.0, 0)
    for got in (vp.synthesize_host(params, ids, frames), g.Plan.synthesize_host(vp, params, frames)):
        for w, x in zip(want, got):
            assert np.array_equal(w, x)
