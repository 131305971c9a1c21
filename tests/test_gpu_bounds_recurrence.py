"""The resampler's output ranges carried forward by running remainder (csrc/vtm_kernel_v2.inc: stage_bounds,
csrc/vtm_design.hpp: src_bounds_*) instead of divided out per chunk, in the shapes bounds_by_recurrence() names (float, four
rows, SectionDelay 2 and 3) and in model 5's double class, and the divisions everywhere else: a wrong range drops or repeats
output samples, so every case is the oracle's samples, bit for bit in float and to the parity rules in fp64 and mixed.

The control rate is 2000 Hz (20 internal steps per frame at SectionDelay 2, fewer than the shortest chunk, 32 steps), so
that utterances of a few frames end inside the first, second, seventh and ninth chunk of a workgroup:

    ragged      four utterances of 1, 2, 7 and 9 chunks, every last chunk partial, in one launch with four rows forced at
                44.1 kHz out (one ragged four-row workgroup), float, mixed and fp64
    down        the same four at 22.05 kHz out (time_inc > 65536; four rows of 1024-sample rings do not fit the LDS, so
                the launch takes two rows: two ragged workgroups), float and fp64
    one row     batch 1, 3 chunks, on the one-row shape
    stream      four utterances pushed in lockstep in three uneven pieces whose step_base values are no multiples of the
                chunk, against the one-shot launch bit for bit and against the oracle: at SectionDelay 2 (two rows, as
                float streams launch there) and at SectionDelay 3 (four rows: the running remainder from a step_base)
    model 5     one launch of its float class, bit for bit, and of its double class, to model 5's parity rule"""
import functools

import numpy as np
import pytest

import oracle
import tracks
from device_io import run_batch_device
from gama_tts_amd import capi
from parity_rules import TOL, check_model5, within
from shape_matrix_cases import chunk_length, launch_shape, stream_launch_shape
from voice_cases import male_plan, model5_plan, oracle_config, padded, push_in_pieces

pytestmark = pytest.mark.gpu

CRATE = 2000.0
DELAY = 2
CHUNKS = (1, 2, 7, 9)
STREAM_PIECES = (3, 1, 5)
PRECISIONS = {"f32": capi.PRECISION_F32, "mixed": capi.PRECISION_MIXED, "f64": capi.PRECISION_F64}


def frames_for(chunks, steps, chunk):
    """The fewest frames of `steps` steps that end inside chunk number `chunks` (a partial last chunk)."""
    return next(f for f in range(1, 10 * chunks * chunk) if (f * steps + chunk - 1) // chunk == chunks and (f * steps) % chunk)


@functools.lru_cache(maxsize=None)
def utterances(frames):
    return tuple(tracks.random_track(f, 6100 + i, i % 2 == 0) for i, f in enumerate(frames))


@functools.lru_cache(maxsize=None)
def reference(rate, pname, frames, delay=DELAY):
    """The oracle's samples of utterances(frames) at 2000 control frames per second (computed once per case)."""
    cfg = oracle_config("male", rate, delay, 0, PRECISIONS[pname])
    out = tuple(oracle.synthesize(cfg, u, CRATE) for u in utterances(frames))
    for r in out:
        r.setflags(write=False)
    return out


def check(pname, got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if pname == "f32":
        differing = int((got.view(np.uint32) != ref.view(np.uint32)).sum())
        print("%s: %d samples, %d differing bit patterns" % (what, ref.size, differing))
        assert TOL[PRECISIONS[pname]] == 0.0 and differing == 0, what
    else:
        peak = float(np.abs(ref).max())
        print("%s: %d samples, largest difference %.3g of the peak" % (what, ref.size, float(np.abs(got.astype(np.float64) - ref).max()) / peak))
        assert within(got, ref, TOL[PRECISIONS[pname]]), what


@pytest.mark.parametrize("rate,pname,rows", [(44100.0, "f32", 4), (44100.0, "mixed", 4), (44100.0, "f64", 4), (22050.0, "f32", 2), (22050.0, "f64", 2)],
                         ids=["up-f32", "up-mixed", "up-f64", "down-f32", "down-f64"])
def test_a_ragged_workgroup_is_the_oracle(rate, pname, rows):
    plan = male_plan(rate=rate, delay=DELAY, crate=CRATE, precision=PRECISIONS[pname], rows=4)
    assert bool(plan.info.upsampling) == (rate > 30000.0) and (plan.info.time_register_increment > 65536) == (rate < 30000.0)
    assert launch_shape(plan, len(CHUNKS))[0] == rows
    chunk, steps = chunk_length(plan, len(CHUNKS)), int(plan.info.control_steps)
    frames = tuple(frames_for(n, steps, chunk) for n in CHUNKS)
    assert [(f * steps + chunk - 1) // chunk for f in frames] == list(CHUNKS)
    params, counts_in = padded(list(utterances(frames)))
    audio, counts = run_batch_device(plan, params, counts_in, plan.output_capacity(params.shape[1]))
    for b, ref in enumerate(reference(rate, pname, frames)):
        assert counts[b] == ref.size, (b, counts[b], ref.size)
        check(pname, audio[b, : counts[b]], ref, "%g Hz %s utterance of %d chunks of %d" % (rate, pname, CHUNKS[b], chunk))
        assert not audio[b, counts[b]:].any(), b
    plan.close()


def test_one_row_of_three_chunks_is_the_float_oracle():
    plan = male_plan(rate=44100.0, delay=DELAY, crate=CRATE, precision=capi.PRECISION_F32, rows=1)
    assert launch_shape(plan, 1)[0] == 1
    chunk, steps = chunk_length(plan, 1), int(plan.info.control_steps)
    frames = (frames_for(3, steps, chunk),)
    params, counts_in = padded(list(utterances(frames)))
    audio, counts = run_batch_device(plan, params, counts_in, plan.output_capacity(params.shape[1]))
    ref = reference(44100.0, "f32", frames)[0]
    assert counts[0] == ref.size
    check("f32", audio[0, : counts[0]], ref, "one row, 3 chunks of %d" % chunk)
    plan.close()


@pytest.mark.parametrize("delay,rows", [(2, 2), (3, 4)], ids=["d2-two-rows", "d3-four-rows"])
def test_a_stream_in_three_uneven_pieces_is_the_one_shot_launch(delay, rows):
    """Four rows forced.  SectionDelay 2: a float stream keeps the one-row ring and launches with two rows (the divisions);
    SectionDelay 3: four rows, the running remainder started from a step_base other than 0."""
    plan = male_plan(rate=44100.0, delay=delay, crate=CRATE, precision=capi.PRECISION_F32, rows=4)
    assert stream_launch_shape(plan, 4)[0] == rows
    steps, total = int(plan.info.control_steps), sum(STREAM_PIECES)
    bases = np.cumsum(STREAM_PIECES)[:-1] * steps
    assert all(b % c for b in bases for c in (32, 36, 48, 72, 96, 144)), bases  # (no chunk length divides them)
    frames = (total,) * 4
    batch = np.stack(utterances(frames))
    outs, peaks = push_in_pieces(plan, batch, np.array(frames, dtype=np.int32), STREAM_PIECES)
    audio, counts = run_batch_device(plan, batch, np.array(frames, dtype=np.int32), plan.output_capacity(total))
    for b, ref in enumerate(reference(44100.0, "f32", frames, delay)):
        assert counts[b] == ref.size
        check("f32", audio[b, : counts[b]], ref, "one-shot utterance %d" % b)
        check("f32", outs[b], audio[b, : counts[b]], "stream utterance %d" % b)
        assert peaks[b] == np.abs(ref).max(), b
    plan.close()


@pytest.mark.parametrize("float_class", (True, False), ids=("float", "double"))
def test_model_5_is_its_oracle(float_class):
    plan = model5_plan("male", float_class=float_class)
    params = tracks.random_tracks(2, 9, seed0=6200, consonant_heavy=True)
    audio, counts, _ = plan.synthesize_host(params)
    for b in range(2):
        ref, _ = oracle.synthesize5(oracle.male5_config(48000.0, 1 if float_class else 0), params[b])
        assert counts[b] == ref.size
        if float_class:
            check("f32", audio[b, : ref.size], ref, "model 5 float utterance %d" % b)
        else:
            check_model5(audio[b, : ref.size], ref)
    plan.close()
