"""The float decimator pass with its coefficients as literals (csrc/vtm_design.hpp: kGlottalFirF32) and, forced through
the diagnostics library, with the generic tap loop over the plan's coefficients in LDS: both bit for bit the float oracle,
signs of zero included (the samples are compared as bit patterns, and one utterance is silent: its decimator adds
0 + (+-0 product) 47 times, and only the first add in the reference's form leaves the sign the reference has).

    one-shot    forced rows 1, 2 and 4 x SectionDelay 1 and 2 x {literals, generic loop}, five utterances of 0, 1, 2, 5 and 3
                frames.  A frame is 160 internal steps, so the five give the first chunk's zero pre-roll, several chunk
                boundaries and a partial last chunk at every chunk length (144, 96 and 48 steps), and a second four-row
                workgroup with a single row.  The 5-frame one is silent.  (Two of the six shapes, one row at SectionDelay 1 and
                two rows at SectionDelay 2, measured slower with literals and keep the plan's coefficients in SGPRs,
                csrc/vtm_kernel_v2.inc: fir_literal_taps; they have no literal path to switch off, and both of their cases run
                that one loop.)
    voices      male + female in one four-row launch, on the literal path and with the generic loop forced.
    stream      a 5-frame utterance pushed in two pieces, on the literal path."""
import functools

import numpy as np
import pytest

import gama_tts_amd as g
import oracle
import tracks
from device_io import run_batch_device, run_voices_device
from gama_tts_amd import capi
from parity_rules import TOL, within
from voice_cases import configs, male_plan, oracle_config, padded, push_in_pieces

pytestmark = pytest.mark.gpu

RATE = 44100.0
DELAYS = (1, 2)
ROWS = (1, 2, 4)
FRAMES = (0, 1, 2, 5, 3)
VOICE_NAMES = ("male", "female")
VOICE_IDS = (0, 1, 1, 0, 1)


@functools.lru_cache(maxsize=None)
def utterances():
    silent = tracks.const_track(5)
    silent[:, 1:4] = 0.0  # glottal, aspiration and frication volume 0
    return (np.zeros((0, 16), np.float32), tracks.random_track(1, 5101), tracks.random_track(2, 5102, True), silent,
            tracks.random_track(3, 5103, True))


@functools.lru_cache(maxsize=None)
def reference(delay, voice="male"):
    """The float oracle's samples of the five utterances under a voice (computed once, shared by every test)."""
    cfg = oracle_config(voice, RATE, delay, 0, capi.PRECISION_F32)
    out = tuple(oracle.synthesize(cfg, u) for u in utterances())
    for r in out:
        r.setflags(write=False)
    return out


def same_bits(got, ref):
    assert TOL[capi.PRECISION_F32] == 0.0 and within(got, ref, TOL[capi.PRECISION_F32])
    return got.shape == ref.shape and np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def test_the_silent_utterance_is_zeros_of_the_reference_sign():
    ref = reference(2)[3]
    assert ref.size and not ref.any()  # (+0.0 or -0.0 each: same_bits compares the sign)


@pytest.mark.parametrize("generic", (False, True), ids=("literals", "generic"))
@pytest.mark.parametrize("delay", DELAYS)
@pytest.mark.parametrize("rows", ROWS)
def test_five_short_utterances_are_the_float_oracle_bit_for_bit(rows, delay, generic):
    plan = male_plan(rate=RATE, delay=delay, precision=capi.PRECISION_F32, rows=rows)
    assert plan.uses_fir_literals()
    if generic:
        plan.force_generic_fir()
        assert not plan.uses_fir_literals()
    params, frames = padded(list(utterances()))
    assert tuple(frames.tolist()) == FRAMES
    audio, counts = run_batch_device(plan, params, frames, plan.output_capacity(params.shape[1]))
    for b, ref in enumerate(reference(delay)):
        got = audio[b, : counts[b]]
        print("rows %d delay %d %s utterance %d frames %d count %5d differing bit patterns %d"
              % (rows, delay, "generic" if generic else "literals", b, frames[b], counts[b],
                 int((got.view(np.uint32) != ref.view(np.uint32)).sum()) if got.size == ref.size else -1))
        assert counts[b] == ref.size, (b, counts[b], ref.size)
        assert same_bits(got, ref), b
        assert not audio[b, counts[b]:].any(), b
    plan.close()


@pytest.mark.parametrize("generic", (False, True), ids=("literals", "generic"))
def test_two_voices_in_one_four_row_launch_are_the_float_oracle(generic):
    delay = 2
    plan = g.VoicesPlan(configs(RATE, delay, capi.PRECISION_F32, 0, names=VOICE_NAMES), 250.0, 0, diagnostics=True, rows=4)
    assert plan.uses_fir_literals()
    if generic:
        plan.force_generic_fir()
    params, frames = padded(list(utterances()))
    ids = np.array(VOICE_IDS, dtype=np.int32)
    audio, counts, maxabs = run_voices_device(plan, params, ids, frames, plan.voices_output_capacity(params.shape[1]))
    for b, v in enumerate(VOICE_IDS):
        ref = reference(delay, VOICE_NAMES[v])[b]
        assert counts[b] == ref.size, (b, counts[b], ref.size)
        assert same_bits(audio[b, : counts[b]], ref), b
        assert maxabs[b] == (np.abs(ref).max() if ref.size else 0.0), b
    plan.close()


def test_a_stream_pushed_in_two_pieces_is_the_float_oracle():
    delay = 2
    plan = male_plan(rate=RATE, delay=delay, precision=capi.PRECISION_F32, diagnostics=True)
    assert plan.uses_fir_literals()
    track = tracks.random_track(5, 5104, True)
    outs, peaks = push_in_pieces(plan, track[None], np.array([5], dtype=np.int32), (3, 2))
    ref = oracle.synthesize(oracle_config("male", RATE, delay, 0, capi.PRECISION_F32), track)
    assert same_bits(outs[0], ref)
    assert peaks[0] == np.abs(ref).max()
    plan.close()
