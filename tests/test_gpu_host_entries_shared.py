"""The padded and the packed host entries share one slice pipeline and one set of per-utterance scratch in the plan
(gvtm_synthesize_{batch,voices}_host*, gvtm_synthesize_packed_host*).  On the float plan of the male voice: the two kinds of
call alternate on one plan while that scratch grows and shrinks, each giving what a fresh plan of its own gives; the padded
layout runs more slices than the packed layout has staging sets (a driver that also rotates sets must not make a layout
without sets wait on anything); and the same with five voices and bad voice ids.  Everything with array_equal."""
import numpy as np
import pytest

import gama_tts_amd as g
from gama_tts_amd import capi
import oracle
from device_io import run_batch_device, run_voices_device
from test_gpu_host_pipeline import _pcm_rule, _ragged
from test_gpu_packed import UP_AND_DOWN, run_packed, set_bytes, utterances_of
from voice_cases import configs, male_plan, padded

pytestmark = pytest.mark.gpu


def assert_same(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


def test_padded_and_packed_calls_alternate_on_one_plan():
    shared = male_plan(precision=capi.PRECISION_F32)
    limit = 3 * set_bytes(shared, [20], 2) + 1  # mostly one-utterance slices: the three sets rotate many times
    few = padded(utterances_of((7, 0, 14, 3, 9), 5100))
    many = _ragged(2100, 14, 5200)  # three slices
    ragged = utterances_of(UP_AND_DOWN, 4100)

    def padded_pcm16(plan):
        return plan.synthesize_host_pcm16(*few)

    def packed_pcm16(plan):
        return run_packed(plan, ragged, None, np.int16)

    def padded_float(plan):
        return plan.synthesize_host(*many)

    def fresh(call):
        plan = male_plan(precision=capi.PRECISION_F32)
        plan.set_staging_limit(limit)
        return call(plan)

    shared.set_staging_limit(limit)
    want = {}
    for call in (padded_pcm16, packed_pcm16, padded_float, packed_pcm16, padded_pcm16):
        if call not in want:
            want[call] = fresh(call)
            assert want[call][0].any()  # (there is sound to compare)
        assert_same(call(shared), want[call])
        st = shared.packed_stats()
        assert st.staging_bytes <= limit == st.limit
    assert st.slices > 3 and st.staging_bytes > 0  # (of the last packed call: the sets did rotate)


def test_padded_pipeline_beyond_three_slices():
    """4100 utterances = four per workgroup x 256 compute units four times over and four utterances more: five slices."""
    batch, max_frames = 4100, 6
    params, frames = _ragged(batch, max_frames, 5300)
    frames[-4:] = [max_frames, 0, 1, 3]  # the last slice
    plan = male_plan(precision=capi.PRECISION_F32)
    audio, counts, maxabs = plan.synthesize_host(params, frames)
    pcm, counts16, maxabs16, scales = plan.synthesize_host_pcm16(params, frames)
    device, device_counts = run_batch_device(plan, params, frames, audio.shape[1])
    assert np.array_equal(counts, device_counts) and np.array_equal(counts16, device_counts) and np.array_equal(maxabs16, maxabs)
    assert audio[:1024].any() and audio[4096:].any()  # (the first slice sounds and the last)
    beyond = np.arange(audio.shape[1])[None, :] >= counts[:, None]
    assert np.array_equal(audio, np.where(beyond, np.float32(0.0), device))
    want16 = np.zeros_like(pcm)
    for b in range(batch):
        n = int(counts[b])
        scale = np.float32(oracle.output_scale(device[b, :n])) if n else np.float32(0.0)
        assert np.float32(scales[b]) == scale and maxabs[b] == (np.abs(device[b, :n]).max() if n else 0.0), b
        want16[b, :n] = _pcm_rule(device[b, :n], scale)
    assert np.array_equal(pcm, want16)


def test_five_voices_through_three_slices_with_bad_ids():
    batch, max_frames = 2100, 14
    params, frames = _ragged(batch, max_frames, 5400)
    plan = g.VoicesPlan(configs(precision=capi.PRECISION_F32), 250.0, 0)
    ids = (np.arange(batch) % 5).astype(np.int32)
    bad = [1030, 2099]  # in the second slice and the last utterance of the third
    ids[bad] = [-1, plan.n_voices]
    frames[bad] = max_frames  # (they would sound)
    audio, counts, maxabs = plan.synthesize_host(params, ids, frames)
    device, device_counts, device_maxabs = run_voices_device(plan, params, ids, frames, audio.shape[1])
    assert np.array_equal(counts, device_counts) and np.array_equal(maxabs, device_maxabs)
    assert (counts[bad] == -1).all() and (np.delete(counts, bad) >= 0).all() and not audio[bad].any()
    beyond = np.arange(audio.shape[1])[None, :] >= counts[:, None]
    assert np.array_equal(audio, np.where(beyond, np.float32(0.0), device))
    assert all(audio[ids == v].any() for v in range(5))
