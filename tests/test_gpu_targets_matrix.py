"""The targets variant of every shape of vtm_synth_kernel a launch can be forced to, against the oracle on the device, on
lists whose points sit ON the edges of the targets driver.

vtm_synth_kernel is compiled three times per shape: from frames, with kVoicesFlag and with kTargetsFlag.  The first two have
their matrices (test_gpu_shape_matrix.py, test_gpu_voices_matrix.py); the targets tests go along lines through the shape
space, and their lists (targets_cases.spoken_lists) sit off every chunk edge and every block of four by design.  The targets
driver is the part of the kernel that follows the shape: stage_interp walks first = tg_base + c * C in blocks of four steps,
at a tick offset that depends on the parameter (0 to 2, 3 to 6, 7 to 15), and runs the cursors' bookkeeping only for a block
in which some lane's cursor moves; the prologue begins or resumes a walk per row.  C differs from shape to shape and N from
tube to tube, so the same lists meet a chunk edge elsewhere in every cell.  This file goes across: the 79 cells of
shape_matrix_cases.py that launch with the rows forced on them, each in

    one shot    19 utterances (targets_matrix_cases.step_pool: 0, 1, C - 1, C, 2C + 1, a seeded length, N - 1, N + C + 2 and
                2N + 3 steps, tiled) of edge_lists -- in every tick group a point that enters on kC and on kC - 1, one that
                leaves there while the enter cursor is idle, both cursors at one step, both in one block of four at
                different steps, three points in one block, points at S - 1, S and S + 1 -- into a guard-filled buffer:
                rows and C as the hooks answer, every status 0, every count gvtm_targets_output_count's and the oracle's,
                samples within parity_rules.TOL of the oracle at control rate = internal rate on gvtm_targets_apply_host's
                frames (float: bit-identical; the bar test_gpu_shape_matrix.py holds its launch (b) to), maxabs the largest
                sample, the guard intact behind every count, samples finite, copies bit for bit their first occurrence;
                float cells: also bit for bit the frames entry on a plan of one step per frame fed those frames;
    a stream    five utterances of N + 3C + 70 steps pushed in lockstep in pieces of 1, 11, 13, C + 1, N - 1, 2C + 12 and
                the 33 that are left, the lists with points around every step a launch of the session resumes at as well:
                samples and maxabs bit for bit the one-shot launch of the same plan; held to the rows
                gvtm_debug_stream_launch_shape answers (the 7 cells of STREAM_FALL_BACK run as two rows and assert it);
    voices      the 34 cells of the `mixed` mix of voices_matrix_cases.py that keep their rows (male + female + baby: both
                converter directions and three N in one launch): 19 shuffled utterances through
                gvtm_synthesize_targets_voices_device, each made with its own voice's N, bit for bit a one-voice targets
                plan of its voice forced to the launched rows and within TOL of the oracle; a twentieth with voice id 3
                fails alone with status 5 and leaves its row untouched.

tests/test_targets_matrix_cases.py (CPU) holds the table to what it claims: no cell and no coincidence left out."""
import numpy as np
import pytest

import gama_tts_amd as g
import oracle
import voices_matrix_cases as vm
from gama_tts_amd import capi
from parity_rules import TOL, check_batch, peak_err, within
from shape_matrix_cases import (BATCH, CELLS, FALL_BACK, LAUNCHABLE, POOL, STREAM_FALL_BACK, cell_id, chunk_length, float_model, launch_shape,
                                plan_of, seed_of, stream_launch_shape, stream_rows)
from targets_io import guard_behind_counts, run_targets
from targets_matrix_cases import (BAD_VOICE, GROUPS, LETTERS, STREAM_BATCH, VOICE_CELLS, coincidences, edge_lists, host_frames, oracle_voices,
                                  pool_lists, resume_edges, run_frames, slice_lists, step_pool, stream_bases, stream_pieces, stream_total,
                                  tiled_steps, voices_case)

pytestmark = pytest.mark.gpu

IDS = [cell_id(c) for c in LAUNCHABLE]
each_cell = pytest.mark.parametrize("cell", LAUNCHABLE, ids=IDS)
STREAM_IDS = [cell_id(c) + ("-as-rows2" if cell_id(c) in STREAM_FALL_BACK else "") for c in LAUNCHABLE]
each_stream = pytest.mark.parametrize("cell", LAUNCHABLE, ids=STREAM_IDS)
VOICE_IDS = [vm.cell_id(c) for c in VOICE_CELLS]
each_voices_cell = pytest.mark.parametrize("cell", VOICE_CELLS, ids=VOICE_IDS)
ALL = [LETTERS] * len(GROUPS)


def _against(got, count, peak, ref, precision, what):
    """One utterance's samples, count and maxabs against the oracle's samples to the precision's bar."""
    assert count == ref.size, (what, count, ref.size)
    if precision == capi.PRECISION_F32:
        check_batch(got[None, :], [count], [peak], [ref], True)
    else:
        assert within(got, ref, TOL[precision]), (what, peak_err(got, ref))
        assert peak == (np.abs(got).max() if ref.size else 0.0), what
    assert np.isfinite(got).all() and np.isfinite(peak), what


@each_cell
def test_one_shot_on_the_driver_s_edges(cell):
    plan = plan_of(cell)
    C, N = chunk_length(plan), plan.targets_filter_length()
    assert launch_shape(plan)[0] == cell.rows and bool(plan.info.upsampling) == (cell.direction == "up")
    pool = step_pool(C, N, seed_of(cell))
    lists = pool_lists(C, N, pool, seed_of(cell))
    assert coincidences(lists[int(np.argmax(pool))], C, N, int(pool.max())) == ALL  # (what this case is for)
    steps, idx = tiled_steps(pool)
    audio, counts, maxabs, statuses = run_targets(plan, [lists[t] for t in idx], steps)
    assert not statuses.any(), statuses
    rate = plan.info.internal_rate_hz
    frames = [host_frames(plan, lists[t], int(pool[t])) for t in range(POOL)]
    refs = oracle.synthesize_many([(frames[t], cell.rate, cell.delay, cell.layout, float_model(cell), rate) for t in range(POOL)])
    for t in range(POOL):
        got = audio[t, : refs[t].size]
        print("%s steps %5d count %6d peak error %.3g" % (cell_id(cell), pool[t], counts[t], peak_err(got, refs[t]) if refs[t].size and counts[t] == refs[t].size else 0.0))
        assert counts[t] == plan.targets_output_count(int(pool[t])), (t, int(pool[t]))
        _against(got, counts[t], maxabs[t], refs[t], cell.precision, (t, int(pool[t])))
    assert guard_behind_counts(audio, counts)
    for b in range(POOL, BATCH):
        assert counts[b] == counts[idx[b]] and maxabs[b].tobytes() == maxabs[idx[b]].tobytes(), (b, idx[b])
        assert audio[b].tobytes() == audio[idx[b]].tobytes(), (b, idx[b])
    if float_model(cell):
        # the same bytes as the frames route: a plan of one step per frame of the same cell, fed the host rule's frames
        today = plan_of(cell, crate=rate)
        assert today.info.control_steps == 1 and today.info.internal_rate_hz == rate and launch_shape(today)[0] == cell.rows
        t_audio, t_counts, t_maxabs = run_frames(today, [frames[t] for t in idx], steps)
        assert t_counts.tolist() == counts.tolist() and t_maxabs.tobytes() == maxabs.tobytes()
        for b in range(BATCH):
            assert t_audio[b, : counts[b]].tobytes() == audio[b, : counts[b]].tobytes(), (b, int(steps[b]))


@each_stream
def test_stream_in_lockstep_is_the_one_shot_launch(cell):
    plan = plan_of(cell)
    C, N = chunk_length(plan), plan.targets_filter_length()
    rows, ring, lds = stream_launch_shape(plan, STREAM_BATCH)
    assert rows == stream_rows(cell) and (rows == 2 and cell.rows == 4) == (cell_id(cell) in STREAM_FALL_BACK) and lds <= 160 * 1024, (rows, ring, lds)
    total, pieces = stream_total(C, N), stream_pieces(C, N)
    extra = resume_edges(stream_bases(pieces), N)  # (and the steps around every resume of this session)
    utterances = [edge_lists(C, N, total, seed_of(cell) + 50 + b, extra) for b in range(STREAM_BATCH)]
    assert all(coincidences(u, C, N, total) == ALL for u in utterances)
    audio, counts, maxabs, statuses = run_targets(plan, utterances, [total] * STREAM_BATCH)
    assert not statuses.any() and guard_behind_counts(audio, counts)
    stream = g.Stream(plan, STREAM_BATCH)
    outs, done = [[] for _ in range(STREAM_BATCH)], 0
    for piece in pieces:
        got = stream.push_targets([slice_lists(u, done, piece) for u in utterances], piece)
        for b in range(STREAM_BATCH):
            outs[b].append(got[b])
        done += piece
    assert done == total
    tail, peaks = stream.finish()
    for b in range(STREAM_BATCH):
        whole = np.concatenate(outs[b] + [tail[b]])
        assert whole.size == counts[b] == plan.targets_output_count(total) > 0, (b, whole.size, counts[b])
        assert whole.tobytes() == audio[b, : counts[b]].tobytes(), b
        assert peaks[b].tobytes() == maxabs[b].tobytes() and peaks[b] == np.abs(whole).max(), b
    assert len({audio[b, : counts[b]].tobytes() for b in range(STREAM_BATCH)}) == STREAM_BATCH  # (five utterances)


@each_voices_cell
def test_voices_every_utterance_under_its_own_voice_s_filter(cell):
    plan = vm.voices_plan(cell)
    case = voices_case(cell, plan)
    batch = len(case.step_counts)
    assert vm.voices_launch_shape(plan, batch)[0] == vm.rows_of(cell) == cell.rows
    audio, counts, maxabs, statuses = run_targets(plan, case.utterances, case.step_counts, case.voice_ids)
    assert statuses.tolist() == [BAD_VOICE if b == case.bad else 0 for b in range(batch)], statuses
    assert counts[case.bad] == -1 and maxabs[case.bad] == 0.0
    assert guard_behind_counts(audio, counts)  # (the bad utterance's whole row among them)
    refs = oracle_voices(cell, plan, case)
    for v in range(3):
        mine = [b for b, w in enumerate(case.voice_ids) if w == v]
        single = vm.single_plan(cell, v, cell.rows)
        assert single.info.upsampling == vm.upsampling_of(cell)[v] and single.targets_filter_length() == plan.targets_filter_length(v)
        s_audio, s_counts, s_maxabs, s_statuses = run_targets(single, [case.utterances[b] for b in mine], [case.step_counts[b] for b in mine])
        assert not s_statuses.any() and guard_behind_counts(s_audio, s_counts)
        for i, b in enumerate(mine):
            n = int(counts[b])
            got = audio[b, :n]
            print("%s utterance %2d voice %d steps %5d count %6d peak error %.3g"
                  % (vm.cell_id(cell), b, v, case.step_counts[b], n, peak_err(got, refs[b]) if refs[b].size == n and n else 0.0))
            assert n == s_counts[i] == plan.targets_voice_output_count(v, case.step_counts[b]), (b, v, n)
            assert got.tobytes() == s_audio[i, :n].tobytes() and maxabs[b].tobytes() == s_maxabs[i].tobytes(), (b, v, case.step_counts[b])
            _against(got, n, maxabs[b], refs[b], cell.precision, (b, v, case.step_counts[b]))
        single.close()


def test_the_matrix_is_complete():
    """The parametrizations above are the whole tables: the 79 cells that keep their forced rows, each once as a one-shot
    launch and once as a stream (72 with their rows, the 7 named ones as two), and the 34 cells of the `mixed` mix of voices
    that keep theirs; none skipped or expected to fail."""
    assert len(CELLS) == 90 and len(IDS) == 79 == len(set(IDS)) and {cell_id(c) for c in CELLS} - set(IDS) == FALL_BACK
    assert sum(i.endswith("-as-rows2") for i in STREAM_IDS) == 7 == len(STREAM_FALL_BACK) and len(STREAM_IDS) == 79
    assert len(VOICE_IDS) == 34 == len(set(VOICE_IDS))
    assert {vm.cell_id(c) for c in vm.CELLS if c.mix == "mixed"} - set(VOICE_IDS) == {i for i in vm.VOICES_FALL_BACK if "-mixed-" in i}
    for fn, cells in ((test_one_shot_on_the_driver_s_edges, LAUNCHABLE), (test_stream_in_lockstep_is_the_one_shot_launch, LAUNCHABLE),
                      (test_voices_every_utterance_under_its_own_voice_s_filter, VOICE_CELLS)):
        marks = [m for m in fn.pytestmark if m.name == "parametrize"]
        assert len(marks) == 1 and tuple(marks[0].args[1]) == tuple(cells)
        assert not [m for m in fn.pytestmark if m.name in ("skip", "skipif", "xfail")]
