"""Every shape of vtm_synth_kernel a launch can be forced to, against the oracle on the device.

The kernel bench.py times is a family of template instantiations (csrc/vtm_kernels.hip: with_shape / v2_shape) picked by
precision, SectionDelay, tube layout, utterances per workgroup and the converter's direction; every member has its own
chunk length, tube unroll, record form and ring, and its own way through the kernel's compile-time switches.  The other
GPU tests compare the family with the oracle along a few lines through that space; this one goes across it: the 79
cells of shape_matrix_cases.py that launch with the rows forced on them, each in

    launch (a)  19 ragged utterances at the 250 Hz control rate whose lengths end on a whole chunk, on the shortest and
                on the longest partial chunk that control rate can reach, besides 0, 1 and 2 frames;
    launch (b)  19 ragged utterances at one step per frame: 0, 1, C - 1, C, C + 1, 2C, 2C + 1, 3C - 1 steps, so that the
                last chunk is whole, one step long or one step short, and the flush zeros run over the chunks after it;
    a stream    five utterances of 31 frames pushed in lockstep (shared workgroups) in uneven pieces.  A stream keeps
                the one-row shape's ring for every shape, and with it 7 of the 79 (STREAM_FALL_BACK: fp64 and float, four
                rows, up-sampling, where that ring is 512 samples and not 256) exceed the LDS and launch as two rows: 72
                shapes run as streams, among them the mixed four-row ones on the 512-sample ring; the test holds every
                stream to the rows the table says.

(a) and (b): every pool member against the oracle to the project's bars (parity_rules.TOL: fp64 1e-9 of peak or one
float32 ulp of the sample, mixed 1e-5, float bit-identical), its count exact, maxabs its largest sample, its row zero
beyond its count, every sample finite; every copy of a track bit for bit its first occurrence, whichever workgroup and
DPP row it sits in.  The stream: samples and maxabs bit for bit the one-shot launch of the same plan, which (a) and (b)
tie to the oracle; in float bit for bit the float oracle as well."""
import numpy as np
import pytest

import oracle
from gama_tts_amd import capi
from parity_rules import TOL, peak_err, within
from shape_matrix_cases import (BATCH, CELLS, FALL_BACK, LAUNCHABLE, POOL, STREAM_BATCH, STREAM_FRAMES, STREAM_PIECES, cell_id,
                                chunk_length, float_model, frames_a, frames_b, internal_rate, launch_shape, launches, oracle_job,
                                plan_of, pool_tracks, seed_of, stream_launch_shape, stream_rows, stream_tracks, tiled)
from voice_cases import push_in_pieces

pytestmark = pytest.mark.gpu

IDS = [cell_id(c) for c in LAUNCHABLE]
each_cell = pytest.mark.parametrize("cell", LAUNCHABLE, ids=IDS)


def _against_the_oracle(cell, plan, crate, pool_frames):
    """One launch of the pool tiled to BATCH utterances, held to the oracle (the module's docstring)."""
    assert launch_shape(plan)[0] == cell.rows  # the launch keeps the rows forced on it
    pool_params = pool_tracks(pool_frames, seed_of(cell))
    params, frames, idx = tiled(pool_params, pool_frames)
    audio, counts, maxabs = plan.synthesize_host(params, frames)
    refs = oracle.synthesize_many([oracle_job(cell, pool_params[t, : int(pool_frames[t])], crate) for t in range(POOL)])
    tol = TOL[cell.precision]
    assert np.isfinite(audio).all() and np.isfinite(maxabs).all()
    for t in range(POOL):
        r = refs[t]
        got = audio[t, : r.size]
        print("%s frames %4d count %6d peak error %.3g" % (cell_id(cell), pool_frames[t], counts[t], peak_err(got, r) if r.size else 0.0))
        assert counts[t] == r.size, (t, pool_frames[t], counts[t], r.size)
        assert within(got, r, tol), (t, pool_frames[t], peak_err(got, r))
        assert maxabs[t] == (np.abs(got).max() if r.size else 0.0), (t, pool_frames[t])
        assert not audio[t, r.size:].any(), (t, pool_frames[t])  # the rest of a ragged row comes back zero
    for b in range(POOL, BATCH):
        assert counts[b] == counts[idx[b]] and maxabs[b] == maxabs[idx[b]], (b, idx[b])
        assert np.array_equal(audio[b], audio[idx[b]]), (b, idx[b])


@each_cell
def test_launch_a_chunk_residues_of_the_250_hz_control_rate(cell):
    plan = plan_of(cell)
    assert bool(plan.info.upsampling) == (cell.direction == "up")
    frames = frames_a(chunk_length(plan), int(plan.info.control_steps), seed_of(cell))
    _against_the_oracle(cell, plan, 250.0, frames)


@each_cell
def test_launch_b_one_step_per_frame_around_the_chunk_edges(cell):
    crate = float(internal_rate(cell))
    plan = plan_of(cell, crate)
    assert plan.info.control_steps == 1 and bool(plan.info.upsampling) == (cell.direction == "up")
    _against_the_oracle(cell, plan, crate, frames_b(chunk_length(plan), seed_of(cell)))


@each_cell
def test_stream_in_lockstep_is_the_one_shot_launch(cell):
    plan = plan_of(cell)
    rows, ring, lds = stream_launch_shape(plan)
    assert rows == stream_rows(cell) and ring == launch_shape(plan_of(cell, device=capi.DEVICE_NONE, rows=1))[1] and lds <= 160 * 1024, (rows, ring, lds)
    params = stream_tracks(cell)
    total = np.full(STREAM_BATCH, STREAM_FRAMES, dtype=np.int32)
    whole, counts, maxabs = plan.synthesize_host(params)
    outs, peaks = push_in_pieces(plan, params, total, STREAM_PIECES)
    for b in range(STREAM_BATCH):
        assert outs[b].size == counts[b] > 0, (b, outs[b].size, counts[b])
        assert np.array_equal(outs[b], whole[b, : counts[b]]), b
        assert peaks[b] == maxabs[b] == np.abs(whole[b]).max(), b
    if float_model(cell):
        refs = oracle.synthesize_many([oracle_job(cell, params[b]) for b in range(STREAM_BATCH)])
        for b in range(STREAM_BATCH):
            assert np.array_equal(outs[b], refs[b]), b


def test_the_matrix_is_complete():
    """The parametrization above is the whole table: of the 90 cells the 79 that keep their forced rows, each once and none
    skipped; the other 11, four rows when down-sampling, launch as two rows -- and are exactly the ones the table names."""
    assert len(CELLS) == 90 and len(set(CELLS)) == 90
    keeps = {cell_id(c) for c in CELLS if launches(c)}
    assert len(keeps) == 79 and keeps == set(IDS) and len(IDS) == 79
    assert {cell_id(c) for c in CELLS} - keeps == FALL_BACK and len(FALL_BACK) == 11
    for fn in (test_launch_a_chunk_residues_of_the_250_hz_control_rate, test_launch_b_one_step_per_frame_around_the_chunk_edges,
               test_stream_in_lockstep_is_the_one_shot_launch):
        marks = [m for m in fn.pytestmark if m.name == "parametrize"]
        assert len(marks) == 1 and [cell_id(c) for c in marks[0].args[1]] == IDS
        assert not [m for m in fn.pytestmark if m.name in ("skip", "skipif", "xfail")]
