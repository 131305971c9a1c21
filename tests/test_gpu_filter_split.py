"""The float kernels' post-tube filter stage with its feed-forward half run 64 steps at a time (csrc/vtm_kernel_v2.inc:
stage_f2_split; which shapes take it: filter_split_f2) against the float oracle, bit for bit, and the two code paths against
each other through the two variants of the diagnostics library that force the split off resp. on for every shape that can
take it (lib/libgama_vtm_diag_fsplit0.so, ..._fsplit1.so; csrc/Makefile).

The male voice at 44.1 kHz has 160 internal steps per frame at SectionDelay 2 and 80 at SectionDelay 1; the chunks are 48
(four rows), 96 (two) and 144 steps (one row), the rings of a one-shot launch 256, 512 and 512 samples, a stream's 512
whatever its rows (asserted below through the launch-shape hooks).

    ragged      nine utterances of 0, 1, 1, 2, 2, 3, 5, 5 and 7 frames: the third four-row workgroup has one live row, the
                last chunk of an utterance is 16 or 32 steps in four rows (160 = 3 x 48 + 16, 80 = 48 + 32), and the ring
                wraps and its mirror slots are written again from the second frame on (four rows, SectionDelay 2) resp. by
                the 5- and 7-frame utterances everywhere.  Four rows at SectionDelay 2 and 1, two rows at SectionDelay 2, one
                row at both; counts exact, zeros behind the count.
    silent      an utterance whose three volumes are zero throughout next to three voiced ones in a four-row workgroup:
                the signs of its zeros.
    stream      five utterances of 6 frames in lockstep through the streams of a four-row and a two-row plan, pushed as
                1 + 2 + 3 and as 4 + 2 frames: the radiation filters' states cross launches, and the pushes start at steps
                160, 480 and 640 of a ring of 512.  Both streams launch two rows (four rings of 512 do not fit), a shape
                that takes the split only in the library that forces it on: each case runs on the product's kernels and
                on that library's.
    odd steps   gvtm_synthesize_targets_device at SectionDelay 2 with 1, 2, 3, 5, 47, 48, 49, 95, 97, 257 and 259 steps, in
                one row and in four: the host rule's frames through the oracle at one step per frame.
    both paths  the ragged case and the odd step counts on the two forced libraries: equal to each other (and to the oracle)."""
import contextlib
import ctypes
import functools
import os

import numpy as np
import pytest

import gama_tts_amd as g
import oracle
import targets_cases
import tracks
from device_io import run_batch_device
from gama_tts_amd import capi
from targets_io import run_targets
from voice_cases import male_plan, padded

pytestmark = pytest.mark.gpu

RATE = 44100.0
RAGGED = (0, 1, 1, 2, 2, 3, 5, 5, 7)
SHAPES = [(2, 4), (1, 4), (2, 2), (2, 1), (1, 1)]  # (SectionDelay, rows)
SHAPE_IDS = ["d2-four-rows", "d1-four-rows", "d2-two-rows", "d2-one-row", "d1-one-row"]
CHUNK = {4: 48, 2: 96, 1: 144}
RING = {4: 256, 2: 512, 1: 512}
STEPS_PER_FRAME = {2: 160, 1: 80}
ADOPTED = {(2, 4)}  # the shapes whose product kernel takes the split
ODD_STEPS = (1, 2, 3, 5, 47, 48, 49, 95, 97, 257, 259)
LONGEST = 260


@contextlib.contextmanager
def diagnostics_library(forced):
    """Plans made inside come from the diagnostics library (forced None) or from its variant with the split forced off (0)
    resp. on (1) for every shape that can take it."""
    if forced is None:
        yield
        return
    path = os.path.join(os.path.dirname(capi.library_path(True)), "libgama_vtm_diag_fsplit%d.so" % forced)
    assert os.path.exists(path), path
    saved_lib, saved_env = capi._libs.pop(True, None), os.environ.get("GVTM_DIAG_LIBRARY")
    os.environ["GVTM_DIAG_LIBRARY"] = path
    try:
        yield
    finally:
        capi._libs.pop(True, None)
        if saved_lib is not None:
            capi._libs[True] = saved_lib
        if saved_env is None:
            del os.environ["GVTM_DIAG_LIBRARY"]
        else:
            os.environ["GVTM_DIAG_LIBRARY"] = saved_env


def float_plan(delay, rows):
    return male_plan(rate=RATE, delay=delay, precision=capi.PRECISION_F32, rows=rows)


def launch_shape(plan, batch, stream=False):
    out = (ctypes.c_size_t * 3)()
    rc = plan._lib.gvtm_debug_stream_launch_shape(plan._h, batch, out) if stream else plan._lib.gvtm_debug_launch_shape(plan._h, batch, 0, out)
    assert rc == 0
    return int(out[0]), int(out[1])


def takes_the_split(plan, delay, rows, forced):
    """What the plan's library says about the shape, held to what this file expects of that library."""
    says = plan.filter_split(rows)
    assert says == (int((delay, rows) in ADOPTED) if forced is None else forced), (delay, rows, forced, says)
    return bool(says)


@functools.lru_cache(maxsize=None)
def utterances(frames, seed0=9100):
    return tuple(tracks.random_track(n, seed0 + 17 * i, i % 2 == 1) if n else np.zeros((0, 16), np.float32) for i, n in enumerate(frames))


@functools.lru_cache(maxsize=None)
def reference(frames, delay, seed0=9100):
    """The float oracle's samples of utterances(frames) (computed once, shared, read-only)."""
    cfg = oracle.male_config(RATE, delay, float_model=1)
    out = tuple(oracle.synthesize(cfg, u) for u in utterances(frames, seed0))
    for r in out:
        r.setflags(write=False)
    return out


def same_bits(got, ref):
    return got.shape == ref.shape and np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def one_shot(plan, batch):
    params, counts_in = padded(list(batch))
    audio, counts = run_batch_device(plan, params, counts_in, plan.output_capacity(params.shape[1]))
    return audio, counts


def check_against(audio, counts, refs, what):
    for b, ref in enumerate(refs):
        got = audio[b, : counts[b]]
        print("%s utterance %d count %6d differing bit patterns %d"
              % (what, b, counts[b], int((got.view(np.uint32) != ref.view(np.uint32)).sum()) if got.size == ref.size else -1))
        assert counts[b] == ref.size, (b, counts[b], ref.size)
        assert same_bits(got, ref), b
        assert not audio[b, counts[b]:].any(), b


def ragged_covers_the_edges(plan, delay, rows):
    """The lengths do what the file's header says of them, by the shape's real chunk and ring."""
    chunk = int(plan._lib.gvtm_debug_chunk_length(plan._h, len(RAGGED)))
    assert (rows, chunk) == (rows, CHUNK[rows]) and launch_shape(plan, len(RAGGED)) == (rows, RING[rows])
    steps = [n * STEPS_PER_FRAME[delay] for n in RAGGED]
    assert plan.info.control_steps == STEPS_PER_FRAME[delay]
    assert max(steps) > RING[rows] + 32  # the ring wraps, and the slots of its mirror are written a second time
    if rows == 4:
        assert STEPS_PER_FRAME[delay] % chunk in (16, 32) and len(RAGGED) % 4 == 1
        assert delay != 2 or all(s > RING[rows] + 32 for s in steps if s > STEPS_PER_FRAME[delay])  # ... from the second frame on


@pytest.mark.parametrize("delay,rows", SHAPES, ids=SHAPE_IDS)
def test_nine_ragged_utterances_are_the_float_oracle(delay, rows):
    plan = float_plan(delay, rows)
    takes_the_split(plan, delay, rows, None)
    ragged_covers_the_edges(plan, delay, rows)
    audio, counts = one_shot(plan, utterances(RAGGED))
    check_against(audio, counts, reference(RAGGED, delay), "ragged delay %d rows %d" % (delay, rows))
    plan.close()


def test_a_silent_utterance_keeps_the_signs_of_its_zeros():
    frames = (3, 3, 3, 3)
    silent = tracks.const_track(3)
    silent[:, 1:4] = 0.0  # glottal, aspiration and frication volume 0
    voiced = utterances(frames, 9300)
    batch = (voiced[0], np.asarray(silent, dtype=np.float32), voiced[2], voiced[3])
    cfg = oracle.male_config(RATE, 2, float_model=1)
    refs = [oracle.synthesize(cfg, u) for u in batch]
    assert refs[1].size and not refs[1].any() and all(r.any() for i, r in enumerate(refs) if i != 1)
    plan = float_plan(2, 4)
    assert takes_the_split(plan, 2, 4, None)
    audio, counts = one_shot(plan, batch)
    check_against(audio, counts, refs, "silent")  # (as uint32: +0.0 and -0.0 differ)
    plan.close()


@pytest.mark.parametrize("pieces", [(1, 2, 3), (4, 2)], ids=["1+2+3", "4+2"])
@pytest.mark.parametrize("rows", (4, 2))
@pytest.mark.parametrize("forced", (None, 1), ids=["product", "forced-on"])
def test_a_stream_pushed_in_pieces_is_the_one_shot_result(forced, rows, pieces):
    """(A stream keeps the one-row shape's ring of 512 samples for every shape, and four such rings do not fit next to this
    voice's records: the stream of the four-row plan launches two rows, whose kernel takes the split only where it is forced
    on -- so the forced library is what carries the split's filter states across launches here.)"""
    frames = (6,) * 5
    with diagnostics_library(forced):
        plan = float_plan(2, rows)
        takes_the_split(plan, 2, rows, forced)
        stream_rows, ring = launch_shape(plan, len(frames), stream=True)
        assert (stream_rows, ring) == (2, 512) and (forced is None or plan.filter_split(stream_rows) == 1)
        starts = np.cumsum((0,) + pieces)[1:-1] * STEPS_PER_FRAME[2]
        assert all(s % ring for s in starts) and 6 * STEPS_PER_FRAME[2] > ring  # pushes begin inside the ring, and it wraps
        refs = reference(frames, 2, 9500)
        batch = np.stack(utterances(frames, 9500))
        audio, counts = one_shot(plan, utterances(frames, 9500))
        st = g.Stream(plan, len(frames))
        parts, at = [], 0
        for n in pieces:
            parts.append(st.push(batch[:, at: at + n]))
            at += n
        tails, peaks = st.finish()
        st.close()
        for b, ref in enumerate(refs):
            got = np.concatenate([p[b] for p in parts] + [tails[b]])
            assert same_bits(got, ref), b
            assert same_bits(got, audio[b, : counts[b]]), b
            assert peaks[b] == np.abs(ref).max(), b
        plan.close()


# ---- odd step counts, through the targets entry ----

@functools.lru_cache(maxsize=None)
def spoken(seed):
    """Utterance `seed`'s 16 target lists and, once for LONGEST steps, the host rule's frames (a shorter utterance's are
    their first rows) -- by a design-only plan of the product library."""
    plan = male_plan(rate=RATE, delay=2, precision=capi.PRECISION_F32, device=capi.DEVICE_NONE)
    lists = targets_cases.spoken_lists(LONGEST, seed, stride=37)
    frames, status = capi.targets_apply_host(plan, lists, LONGEST)
    plan.close()
    assert status == 0
    frames.setflags(write=False)
    return lists, frames


@functools.lru_cache(maxsize=None)
def odd_reference(seed, steps):
    plan = male_plan(rate=RATE, delay=2, precision=capi.PRECISION_F32, device=capi.DEVICE_NONE)
    rate = plan.info.internal_rate_hz
    plan.close()
    cfg = oracle.male_config(RATE, 2, float_model=1)
    assert oracle.derive(cfg, rate).control_steps == 1
    ref = oracle.synthesize(cfg, spoken(seed)[1][:steps], control_rate=rate)
    ref.setflags(write=False)
    return ref


def check_odd_steps(plan, rows):
    assert int(plan._lib.gvtm_debug_chunk_length(plan._h, len(ODD_STEPS))) == CHUNK[rows]
    # (zeros, not the guard pattern, behind the counts: check_against wants them)
    audio, counts, _, statuses = run_targets(plan, [spoken(b)[0] for b in range(len(ODD_STEPS))], ODD_STEPS, peaks=False, fill=0)
    assert not statuses.any()
    refs = [odd_reference(b, s) for b, s in enumerate(ODD_STEPS)]
    for b, s in enumerate(ODD_STEPS):
        assert refs[b].size == plan.targets_output_count(s)
    check_against(audio, counts, refs, "odd steps rows %d" % rows)
    return audio, counts


@pytest.mark.parametrize("rows", (1, 4))
def test_odd_step_counts_from_targets_are_the_float_oracle(rows):
    plan = float_plan(2, rows)
    takes_the_split(plan, 2, rows, None)
    check_odd_steps(plan, rows)
    plan.close()


# ---- both paths ----

@pytest.mark.parametrize("delay,rows", SHAPES, ids=SHAPE_IDS)
def test_the_split_and_the_serial_form_give_the_same_samples(delay, rows):
    got = {}
    for forced in (0, 1):
        with diagnostics_library(forced):
            plan = float_plan(delay, rows)
            assert takes_the_split(plan, delay, rows, forced) == bool(forced)  # (every shape here can take it)
            got[forced] = one_shot(plan, utterances(RAGGED))
            plan.close()
    assert got[0][1].tolist() == got[1][1].tolist()
    assert np.array_equal(got[0][0].view(np.uint32), got[1][0].view(np.uint32))
    check_against(got[1][0], got[1][1], reference(RAGGED, delay), "forced on, delay %d rows %d" % (delay, rows))


@pytest.mark.parametrize("rows", (1, 4))
def test_odd_step_counts_on_both_paths(rows):
    got = {}
    for forced in (0, 1):
        with diagnostics_library(forced):
            plan = float_plan(2, rows)
            assert takes_the_split(plan, 2, rows, forced) == bool(forced)
            got[forced] = check_odd_steps(plan, rows)
            plan.close()
    assert got[0][1].tolist() == got[1][1].tolist()
    assert np.array_equal(got[0][0].view(np.uint32), got[1][0].view(np.uint32))


def test_a_shape_that_cannot_take_the_split_says_so_and_runs_one_code():
    """SectionDelay 3 keeps the record-per-step tube record: forced on or off, its kernel is the product's."""
    frames = (2, 1, 0, 2, 1)
    out = {}
    for forced in (None, 0, 1):
        with diagnostics_library(forced):
            plan = float_plan(3, 4)
            assert plan.filter_split(4) == 0
            out[forced] = one_shot(plan, utterances(frames, 9700))
            plan.close()
    for forced in (0, 1):
        assert out[forced][1].tolist() == out[None][1].tolist()
        assert np.array_equal(out[forced][0].view(np.uint32), out[None][0].view(np.uint32))
