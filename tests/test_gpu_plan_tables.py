"""The float kernels with what the plan fixes once -- the resampler's coefficients by output phase from the plan's table in
device memory (SynthArgs::src_phase) and the static-wavetable flag (SynthArgs::static_wavetable) -- and, forced through the
diagnostics library, with both formed in the kernel again: each bit for bit the float oracle, hence each other.

Which shapes read the table and the flag is the kernel's choice, shape by shape (csrc/vtm_kernel_v2.inc: src_phase_table,
static_wavetable_pass): four rows at SectionDelay 2 take the flag, four rows at SectionDelay 1 and two rows at SectionDelay 2
the table and the flag, one row neither.  The hooks clear the plan's side, so a shape that reads neither runs one code in
all four cases.

    base        four rows at SectionDelay 2, nine utterances of 1, 13, 47, 48, 60, 60, 61, 75 and 75 frames: the third
                workgroup has one row, and with the plan's 8192 phases the phase index wraps after 8192 / 176.4 = 46.4
                frames' worth of outputs, so every utterance from 47 frames on wraps it.  The same nine in two rows at
                SectionDelay 2 (a shape that reads the table), and in four rows at SectionDelay 1 with the four longest
                lengthened to 93, 94, 100 and 100 frames: that plan has 16384 phases, which wrap after 92.9 frames.  Each as the
                plan makes it, with the table cleared, with the flag cleared, and with both cleared.
    shapes      one and two rows at SectionDelay 2 and one, two and four rows at SectionDelay 1, three utterances of 60 frames.
    stream      five utterances of 60 frames in lockstep through a four-row and a two-row stream, pushed as 40 + 20 and as
                50 + 10 frames: the second launch takes over at output 6868 resp. 8453, neither a multiple of 64, one
                before and one behind the wrap at 8192.
    declined    48 kHz out has 32768 phases, above the cap: no table, the kernel forms the coefficients.
    dynamic     a voice with tn_min != tn_max in the four-row shape: the plan does not set the flag, and the wavetable pass
                asks per entry as before."""
import functools

import numpy as np
import pytest

import gama_tts_amd as g
import oracle
import tracks
from device_io import run_batch_device
from gama_tts_amd import capi
from voice_cases import male_plan, padded

pytestmark = pytest.mark.gpu

RATE = 44100.0
BASE_FRAMES = (1, 13, 47, 48, 60, 60, 61, 75, 75)
BASE_FRAMES_D1 = (1, 13, 47, 48, 60, 93, 94, 100, 100)
PHASES = {2: 8192, 1: 16384}  # the male voice at 44.1 kHz, by SectionDelay (tests/test_src_phase_table_cpu.py)
MOVING = dict(glottal_pulse_tn_min=10.0, glottal_pulse_tn_max=40.0)


@functools.lru_cache(maxsize=None)
def utterances(frames):
    return tuple(tracks.random_track(n, 7300 + 17 * i, i % 2 == 1) for i, n in enumerate(frames))


@functools.lru_cache(maxsize=None)
def reference(frames, delay, rate=RATE, overrides=()):
    """The float oracle's samples of utterances(frames) (computed once, shared, read-only)."""
    cfg = oracle.male_config(rate, delay, float_model=1, **dict(overrides))
    out = tuple(oracle.synthesize(cfg, u) for u in utterances(frames))
    for r in out:
        r.setflags(write=False)
    return out


def float_plan(delay, rows, rate=RATE, overrides=None):
    return male_plan(overrides, rate=rate, delay=delay, precision=capi.PRECISION_F32, rows=rows)


def check_one_shot(plan, frames, refs, what):
    params, counts_in = padded(list(utterances(frames)))
    audio, counts = run_batch_device(plan, params, counts_in, plan.output_capacity(params.shape[1]))
    for b, ref in enumerate(refs):
        got = audio[b, : counts[b]]
        print("%s utterance %d frames %d count %6d differing bit patterns %d"
              % (what, b, frames[b], counts[b], int((got.view(np.uint32) != ref.view(np.uint32)).sum()) if got.size == ref.size else -1))
        assert counts[b] == ref.size, (b, counts[b], ref.size)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), b
        assert not audio[b, counts[b]:].any(), b


@pytest.mark.parametrize("generic_src,dynamic_wavetable", [(False, False), (True, False), (False, True), (True, True)],
                         ids=["plan-tables", "generic-src", "dynamic-wavetable", "both-generic"])
@pytest.mark.parametrize("delay,rows,frames", [(2, 4, BASE_FRAMES), (2, 2, BASE_FRAMES), (1, 4, BASE_FRAMES_D1)],
                         ids=["d2-four-rows", "d2-two-rows", "d1-four-rows"])
def test_nine_ragged_utterances_are_the_float_oracle(delay, rows, frames, generic_src, dynamic_wavetable):
    plan = float_plan(delay, rows)
    assert plan.src_phases() == PHASES[delay] and plan.says_static_wavetable()
    # the phase index wraps inside the utterances from `wrap` frames on: the longest ones
    wrap = int(PHASES[delay] * 250.0 / RATE) + 1
    assert plan.output_count(wrap) > PHASES[delay] > plan.output_count(wrap - 1) and wrap in frames and sum(n >= wrap for n in frames) >= 4
    if generic_src:
        plan.force_generic_src()
        assert plan.src_phases() == 0
    if dynamic_wavetable:
        plan.force_dynamic_wavetable()
        assert not plan.says_static_wavetable()
    check_one_shot(plan, frames, reference(frames, delay), "base delay %d rows %d" % (delay, rows))
    plan.close()


@pytest.mark.parametrize("delay,rows", [(2, 1), (2, 2), (1, 1), (1, 2), (1, 4)])
def test_the_other_shapes_are_the_float_oracle(delay, rows):
    frames = (60, 60, 60)
    plan = float_plan(delay, rows)
    assert plan.src_phases() == PHASES[delay] and plan.says_static_wavetable()
    check_one_shot(plan, frames, reference(frames, delay), "delay %d rows %d" % (delay, rows))
    plan.close()


@pytest.mark.parametrize("pieces", [(40, 20), (50, 10)], ids=["boundary-before-the-wrap", "boundary-behind-the-wrap"])
@pytest.mark.parametrize("rows", (4, 2))
def test_a_stream_pushed_in_two_pieces_is_the_one_shot_result(rows, pieces):
    frames = (60,) * 5
    plan = float_plan(2, rows)
    assert plan.src_phases() == PHASES[2]
    one_shot = reference(frames, 2)
    batch = np.stack(utterances(frames))
    st = g.Stream(plan, len(frames))
    first = st.push(batch[:, : pieces[0]])
    second = st.push(batch[:, pieces[0]:])
    tails, peaks = st.finish()
    st.close()
    for b in range(len(frames)):
        boundary = first[b].size  # the output index at which the second launch takes over
        print("rows %d pieces %s utterance %d boundary %d (mod 64: %d) wrap at %d" % (rows, pieces, b, boundary, boundary % 64, PHASES[2]))
        assert boundary % 64 != 0 and (boundary < PHASES[2]) == (pieces[0] == 40), boundary
        got = np.concatenate([first[b], second[b], tails[b]])
        assert got.size == one_shot[b].size, b
        assert np.array_equal(got.view(np.uint32), one_shot[b].view(np.uint32)), b
        assert peaks[b] == np.abs(one_shot[b]).max(), b
    plan.close()


@pytest.mark.parametrize("rows", (4, 2))
def test_a_plan_above_the_cap_runs_without_the_table(rows):
    frames = (60, 60, 60, 13, 1)
    plan = float_plan(2, rows, rate=48000.0)
    assert plan.src_phases() == 0 and plan.says_static_wavetable()
    check_one_shot(plan, frames, reference(frames, 2, 48000.0), "48 kHz rows %d" % rows)
    plan.close()


def test_a_voice_whose_wavetable_follows_the_amplitude_is_exact():
    frames = (60, 47, 13, 60, 1)
    plan = float_plan(2, 4, overrides=MOVING)
    assert plan.src_phases() == PHASES[2] and not plan.says_static_wavetable()
    check_one_shot(plan, frames, reference(frames, 2, RATE, tuple(sorted(MOVING.items()))), "tn_min != tn_max")
    plan.close()
