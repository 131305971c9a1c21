"""The float kernel's parameter-conversion passes (pitch and volumes -> increment and amplitudes, radii -> junction
coefficients, frication -> taps and band-pass design) on the inputs at which their index arithmetic, their constants and
their powf table can go wrong, bit for bit against the float oracle.

    one-shot    forced rows 1, 2, 4 and 8 (diagnostics library) x SectionDelay 1 and 2, a batch of FIVE utterances: a four-row
                group then has three empty rows and an eight-row group three, so the passes see items that do not exist.
                The five are tracks.edge_track(48) -- on both shortcuts of Util::amplitude60dB, both ends of the pitch range,
                frication position 0 and 7 and the radius floor --, random tracks of 13 and 97 frames, a one-frame track
                and a silent one; the ragged lengths leave partial last chunks in every shape.
    stream      the 97-frame track in three pushes against its one-shot output (a stream's passes run without the plan's
                noise table).
    voices      male + female in one four-row launch against their single-voice plans (the voice variant takes its
                constants per voice)."""
import functools

import numpy as np
import pytest

import gama_tts_amd as g
import oracle
import tracks
from gama_tts_amd import capi
from voice_cases import configs, male_plan, oracle_config, padded, push_in_pieces

pytestmark = pytest.mark.gpu

RATE = 44100.0
DELAYS = (1, 2)
ROWS = (1, 2, 4, 8)


@functools.lru_cache(maxsize=None)
def utterances():
    silent = tracks.const_track(5)
    silent[:, 1:4] = 0.0  # glottal, aspiration and frication volume 0: every amplitude takes its first shortcut
    return (tracks.edge_track(48), tracks.random_track(13, 4101, True), tracks.random_track(97, 4102, True),
            tracks.random_track(1, 4103), silent)


@functools.lru_cache(maxsize=None)
def reference(delay):
    """The float oracle's samples of the five utterances (computed once per SectionDelay, shared by every test)."""
    out = tuple(r for r in oracle.synthesize_many([(u, RATE, delay, 0, 1, 250.0) for u in utterances()]))
    for r in out:
        r.setflags(write=False)
    return out


@pytest.mark.parametrize("delay", DELAYS)
@pytest.mark.parametrize("rows", ROWS)
def test_five_ragged_utterances_are_the_float_oracle_bit_for_bit(rows, delay):
    plan = male_plan(rate=RATE, delay=delay, precision=capi.PRECISION_F32, rows=rows)
    params, frames = padded(list(utterances()))
    assert frames.tolist() == [48, 13, 97, 1, 5]
    audio, counts, maxabs = plan.synthesize_host(params, frames)
    for b, ref in enumerate(reference(delay)):
        got = audio[b, : counts[b]]
        print("rows %d delay %d utterance %d frames %2d count %6d differing samples %d"
              % (rows, delay, b, frames[b], counts[b], int((got != ref).sum()) if got.size == ref.size else -1))
        assert counts[b] == ref.size, (b, counts[b], ref.size)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), b
        assert maxabs[b] == np.abs(ref).max() and not audio[b, counts[b]:].any(), b
    plan.close()


@pytest.mark.parametrize("delay", DELAYS)
def test_a_stream_in_three_pushes_is_the_one_shot_output(delay):
    plan = male_plan(rate=RATE, delay=delay, precision=capi.PRECISION_F32, diagnostics=True)
    track = utterances()[2][None]
    outs, peaks = push_in_pieces(plan, track, np.array([97], dtype=np.int32), (31, 48, 18))
    ref = reference(delay)[2]
    assert outs[0].size == ref.size and np.array_equal(outs[0].view(np.uint32), ref.view(np.uint32))
    assert peaks[0] == np.abs(ref).max()
    plan.close()


@pytest.mark.parametrize("delay", DELAYS)
def test_two_voices_in_one_four_row_launch_are_their_single_voice_plans(delay):
    names = ("male", "female")
    cfgs = configs(RATE, delay, capi.PRECISION_F32, 0, names=names)
    plan = g.VoicesPlan(cfgs, 250.0, 0, diagnostics=True, rows=4)
    params, frames = padded(list(utterances()))
    ids = np.array([0, 1, 1, 0, 1], dtype=np.int32)
    audio, counts, maxabs = plan.synthesize_host(params, ids, frames)
    for v, name in enumerate(names):
        sel = np.flatnonzero(ids == v)
        single = g.Plan(cfgs[v], 250.0, 0, diagnostics=True, rows=4)
        s_audio, s_counts, s_maxabs = single.synthesize_host(params[sel], frames[sel])
        for j, b in enumerate(sel):
            assert counts[b] == s_counts[j] and maxabs[b] == s_maxabs[j], (name, b)
            assert np.array_equal(audio[b, : counts[b]].view(np.uint32), s_audio[j, : s_counts[j]].view(np.uint32)), (name, b)
        single.close()
    # ... and the female voice's utterances the float oracle's (the male ones: the test above)
    fem = oracle_config("female", RATE, delay, 0, capi.PRECISION_F32)
    for b in np.flatnonzero(ids == 1):
        ref = oracle.synthesize(fem, utterances()[b])
        assert counts[b] == ref.size and np.array_equal(audio[b, : counts[b]].view(np.uint32), ref.view(np.uint32)), b
    plan.close()
