"""The case table of the shape matrix (shape_matrix_cases.py) held to design-only plans of the diagnostics library, so
that what tests/test_gpu_shape_matrix.py runs on the device is what its docstring says (CPU test).

    the split: 79 of the 90 cells keep the rows forced on them, the 11 of FALL_BACK launch as two rows;
    every cell's internal rate, steps per frame, converter direction and ring (the reference's 1024 when down-sampling,
    otherwise a power of two that holds what the launch asks of it);
    gvtm_debug_chunk_length: a positive multiple of 4 (the scan blocks) no longer than the chunk of the plan's one-row
    shape, whose ring a stream keeps for every shape;
    the rows of every cell's lockstep stream, on the stream's ring: 72 keep theirs, the 7 of STREAM_FALL_BACK launch two;
    one step per frame at control rate = internal rate;
    launch (a)'s frame counts end on the residues they claim, launch (b)'s sit around the chunk edges;
    gvtm_output_count is the oracle's count for every length of both launches, and gvtm_output_capacity holds it."""
import math

import numpy as np

import oracle
from gama_tts_amd import capi
from shape_matrix_cases import (BATCH, CELLS, FALL_BACK, LAUNCHABLE, MAX_FRAMES_A, POOL, STREAM_FALL_BACK, TUBES,
                                cell_id, chunk_length, float_model, frames_a, frames_b, hooks, internal_rate, launch_shape, launches,
                                plan_of, pool_tracks, residues, seed_of, stream_launch_shape, stream_rows, tiled)


def _design(cell, crate=250.0, rows=None):
    return plan_of(cell, crate, capi.DEVICE_NONE, rows)


def test_79_cells_keep_their_rows_and_the_11_named_ones_fall_back_to_two():
    assert len(CELLS) == 90 and len(set(cell_id(c) for c in CELLS)) == 90
    keeps = {cell_id(c) for c in CELLS if launches(c)}
    assert keeps == {cell_id(c) for c in LAUNCHABLE} and len(keeps) == 79
    assert {cell_id(c) for c in CELLS} - keeps == FALL_BACK and len(FALL_BACK) == 11
    for c in CELLS:
        if cell_id(c) in FALL_BACK:
            assert c.rows == 4 and c.direction == "down"
            plan = _design(c)
            assert launch_shape(plan)[0] == 2
            plan.close()


def test_rates_direction_ring_and_chunk_of_every_cell():
    for c in LAUNCHABLE:
        plan, one_row = _design(c), _design(c, rows=1)
        info = plan.info
        assert info.internal_sample_rate == internal_rate(c) and info.control_steps == TUBES[c.delay, c.layout]["steps"], cell_id(c)
        assert bool(info.upsampling) == (c.direction == "up"), cell_id(c)
        rows, ring, lds = launch_shape(plan)
        chunk = chunk_length(plan)
        assert rows == c.rows and lds <= 160 * 1024, cell_id(c)
        assert chunk > 0 and chunk % 4 == 0 and chunk <= chunk_length(one_row), (cell_id(c), chunk)
        if c.rows == 1:
            assert chunk == chunk_length(one_row)
        if c.direction == "down":
            assert ring == 1024, (cell_id(c), ring)
        else:
            # a power of two that holds two chunks, the resampler's history and the flush zeros (csrc/vtm_design.hpp: synth_ring_for)
            assert ring & (ring - 1) == 0 and 2 * chunk + 4 * info.pad_size + 64 <= ring < 1024, (cell_id(c), ring)
        assert ring <= launch_shape(one_row)[1], cell_id(c)  # a stream's ring, the one-row shape's, is never the shorter one
        assert 13 <= info.pad_size <= 48, (cell_id(c), info.pad_size)
        plan.close(), one_row.close()


def test_72_cells_keep_their_rows_as_a_stream_and_the_7_named_ones_launch_two():
    """A lockstep stream launches with its own ring, the one-row shape's: the LDS of the cell's rows must fit with THAT
    ring, or the launch takes half as many.  The table names the cells where it does (STREAM_FALL_BACK); the library decides."""
    falls = set()
    for c in LAUNCHABLE:
        plan, one_row = _design(c), _design(c, rows=1)
        rows, ring, lds = stream_launch_shape(plan)
        own_rows, own_ring, own_lds = launch_shape(plan)
        assert ring == launch_shape(one_row)[1] == stream_launch_shape(one_row)[1] >= own_ring, cell_id(c)
        assert lds <= 160 * 1024 and rows == stream_rows(c), (cell_id(c), rows, lds)
        assert stream_launch_shape(plan, BATCH) == (rows, ring, lds)  # forced rows: whatever the batch
        if rows != c.rows:
            falls.add(cell_id(c))
            # two rows, as the stream of the two-row cell launches; the cell's own rows with the stream's ring do not fit
            two = _design(c, rows=2)
            assert c.rows == 4 and (rows, ring, lds) == stream_launch_shape(two) and ring > own_ring and c.direction == "up", cell_id(c)
            two.close()
        elif ring == own_ring:
            assert lds == own_lds, cell_id(c)
        else:
            assert lds > own_lds, cell_id(c)  # (the mixed four-row shapes on the 512-sample ring, among others)
        plan.close(), one_row.close()
    assert falls == STREAM_FALL_BACK and len(falls) == 7 and len(LAUNCHABLE) - len(falls) == 72
    assert {"mixed-%s-up-rows4" % t for t in ("d1", "d2", "d4", "wide")}.isdisjoint(falls)


def test_chunk_length_hook_answers_for_the_launched_rows():
    """Forced rows that do not fit answer with the chunk of the shape they become; a null plan is refused."""
    for c in CELLS:
        if cell_id(c) in FALL_BACK:
            plan, two = _design(c), _design(c, rows=2)
            assert chunk_length(plan) == chunk_length(two) > 0
            plan.close(), two.close()
    assert hooks().gvtm_debug_chunk_length(None, BATCH) < 0


def test_one_step_per_frame_at_control_rate_equal_internal_rate():
    for c in LAUNCHABLE:
        plan, at_250 = _design(c, float(internal_rate(c))), _design(c)
        assert plan.info.control_steps == 1, cell_id(c)
        assert chunk_length(plan) == chunk_length(at_250), cell_id(c)  # the chunk does not follow the control rate
        plan.close(), at_250.close()


def test_frame_counts_of_both_launches():
    for c in LAUNCHABLE:
        plan = _design(c)
        chunk, steps = chunk_length(plan), int(plan.info.control_steps)
        fa = frames_a(chunk, steps, seed_of(c))
        assert fa.size == POOL == len(set(fa.tolist())) and {0, 1, 2} <= set(fa.tolist()) and fa.max() <= MAX_FRAMES_A, (cell_id(c), fa)
        step = math.gcd(steps, chunk)
        assert set(residues(steps, chunk)) == {0, step % chunk, (chunk - step) % chunk}, cell_id(c)  # all three in reach
        for r in residues(steps, chunk):
            assert 0 <= r < chunk
            assert [f for f in fa if f > 0 and (int(f) * steps) % chunk == r], (cell_id(c), r, fa)
        fb = frames_b(chunk, seed_of(c))
        assert fb.size == POOL == len(set(fb.tolist())) and fb.max() == 3 * chunk - 1 <= 431, (cell_id(c), fb)
        assert {0, 1, chunk - 1, chunk, chunk + 1, 2 * chunk, 2 * chunk + 1, 3 * chunk - 1} <= set(fb.tolist())
        assert (fb[:8] % chunk).tolist() == [0, 1 % chunk, chunk - 1, 0, 1, 0, 1, chunk - 1]
        plan.close()


def test_pool_is_cut_to_its_lengths_and_tiled_over_two_rows_each():
    frames = frames_b(24, 1)
    pool = pool_tracks(frames, 1)
    assert pool.shape == (POOL, 3 * 24 - 1, 16)
    for t in range(POOL):
        assert not pool[t, frames[t]:].any() and (frames[t] == 0 or pool[t, : frames[t]].any())
    params, fc, idx = tiled(pool, frames)
    assert params.shape[0] == fc.size == BATCH and BATCH % 4 and BATCH % 2
    for t in range(POOL):
        at = np.flatnonzero(idx == t)
        assert at.size >= 2 and len(set(at % 2)) == 2 and len(set(at % 4)) >= 2  # two different DPP rows of a two- and a four-row workgroup
        assert all(np.array_equal(params[b], pool[t]) and fc[b] == frames[t] for b in at)


def test_output_capacity_holds_every_count_of_both_launches():
    for c in LAUNCHABLE:
        cfg = oracle.male_config(c.rate, c.delay, c.layout, float_model=float_model(c))
        for crate in (250.0, float(internal_rate(c))):
            plan = _design(c, crate)
            chunk = chunk_length(plan)
            frames = frames_a(chunk, int(plan.info.control_steps), seed_of(c)) if crate == 250.0 else frames_b(chunk, seed_of(c))
            capacity = plan.output_capacity(int(frames.max()))
            for f in frames:
                want = oracle.output_count(cfg, int(f), crate)
                assert plan.output_count(int(f)) == want <= capacity, (cell_id(c), crate, int(f), want, capacity)
            plan.close()
