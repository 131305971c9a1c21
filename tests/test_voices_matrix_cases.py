"""The case table of the voices matrix (voices_matrix_cases.py) held to design-only plans of the diagnostics library and to
the oracle, so that what tests/test_gpu_voices_matrix.py runs on the device is what its docstring says (CPU test).

    the split: 113 of the 135 cells keep the rows forced on them, the 22 of VOICES_FALL_BACK launch as two rows; of the 113,
    the lockstep streams of VOICES_STREAM_FALL_BACK launch as two rows (gvtm_debug_stream_launch_shape on plans of several
    voices: the voice variant on the longest of the voices' stream rings; model 5 stays refused);
    every voice's converter direction per mix, and its steps per frame (the oracle's);
    launch A: every voice's frame counts end on the residues they claim for ITS steps per frame and the launched chunk;
    9 / 10 / 11 utterances per voice leave the stated rows of the last group empty; the extra ones are copies of the
    voice's longest members; launch B has no utterance of voice 0 and the two bad ids;
    gvtm_voice_output_count is the oracle's count for every utterance of both launches, gvtm_voices_output_capacity
    holds it;
    the GPU comparison discriminates: no two utterances of a launch that are not deliberate copies have equal expected
    samples (a row-map or voice mix-up cannot pass), and one fixed track gives different samples under each pair of voices."""
import ctypes
import functools
import itertools
import math

import numpy as np

import oracle
import tracks
from gama_tts_amd import capi
from shape_matrix_cases import MAX_FRAMES_A, POOL, TUBES, hooks, residues
from voice_cases import model5_plan, oracle_config
from voices_matrix_cases import (BATCH_B, CELLS, LAUNCHABLE, MIXES, VOICES_FALL_BACK, VOICES_STREAM_FALL_BACK, batch_a, cell_id,
                                 chunk_of, empty_rows, launch_a, launch_b, oracle_many, oracle_pools, rows_of, single_plan,
                                 stream_case, stream_launch_shape, stream_rows, tube_id, upsampling_of, utterances_per_voice,
                                 voices_launch_shape, voices_plan)

# rows of a voice's last group left empty, voices 0 / 1 / 2 with 9 / 10 / 11 utterances
EMPTY_ROWS = {1: (0, 0, 0), 2: (1, 0, 1), 4: (3, 2, 1)}


@functools.lru_cache(maxsize=None)
def _case(cell):
    """(design-only voices plan of the cell, its launch A)"""
    plan = voices_plan(cell, capi.DEVICE_NONE)
    return plan, launch_a(cell, plan)


def test_113_cells_keep_their_rows_and_the_22_named_ones_fall_back_to_two():
    assert len(CELLS) == 135 and len(set(cell_id(c) for c in CELLS)) == 135
    keeps = set()
    for c in CELLS:
        plan = _case(c)[0]
        rows, ring, lds = voices_launch_shape(plan, batch_a(c))
        assert rows == rows_of(c) and lds <= 160 * 1024, (cell_id(c), rows, lds)
        # one down-sampling voice lays the whole launch's LDS out for the reference's 1024-sample ring
        assert (ring == 1024 if 0 in upsampling_of(c) else ring in (256, 512)), (cell_id(c), ring)
        if rows == c.rows:
            keeps.add(cell_id(c))
        else:
            assert c.rows == 4 and rows == 2 and c.mix in ("mixed", "down") and ring == 1024, cell_id(c)
    assert keeps == {cell_id(c) for c in LAUNCHABLE} and len(keeps) == 113
    assert {cell_id(c) for c in CELLS} - keeps == VOICES_FALL_BACK and len(VOICES_FALL_BACK) == 22
    assert not [i for i in VOICES_FALL_BACK if "-d3-" in i or "-up-" in i or i.startswith("f32-wide")]


def test_lockstep_streams_of_several_voices_launch_with_the_rows_the_table_names():
    """The stream's LDS holds the longest of the voices' single-voice stream rings (each the one-row shape's)."""
    falls = set()
    for c in LAUNCHABLE:
        plan = _case(c)[0]
        batch = (stream_rows(c) + 1) * len(c.names)
        rows, ring, lds = stream_launch_shape(plan, batch)
        rings = []
        for v in range(len(c.names)):
            one = single_plan(c, v, 1, capi.DEVICE_NONE)
            rings.append(stream_launch_shape(one, batch)[1])
            one.close()
        own = voices_launch_shape(plan, batch)
        assert ring == max(rings) >= own[1] and lds <= 160 * 1024 and rows == stream_rows(c), (cell_id(c), rows, ring, lds)
        assert stream_launch_shape(plan, 1000) == (rows, ring, lds)  # forced rows: whatever the batch
        if rows != c.rows:
            falls.add(cell_id(c))
            two = voices_plan(c, capi.DEVICE_NONE, rows=2)
            assert c.rows == 4 and rows == 2 and (rows, ring, lds) == stream_launch_shape(two, batch) and ring > own[1], cell_id(c)
            two.close()
        elif ring == own[1]:
            assert lds == own[2], cell_id(c)
        else:
            assert lds > own[2], cell_id(c)
        ids = stream_case(c)[1]
        assert ids.size == batch and np.bincount(ids).tolist() == [rows + 1] * len(c.names), cell_id(c)
    assert falls == VOICES_STREAM_FALL_BACK
    # model 5 stays refused, a null plan too
    plan5 = model5_plan(device=capi.DEVICE_NONE, diagnostics=True)
    out = (ctypes.c_size_t * 3)()
    assert hooks().gvtm_debug_stream_launch_shape(plan5._h, 5, out) == 4  # GVTM_ERR_UNSUPPORTED
    assert hooks().gvtm_debug_stream_launch_shape(None, 5, out) == 1
    plan5.close()


def test_direction_and_steps_per_frame_of_every_voice():
    pairs = set()
    for c in CELLS:
        plan = _case(c)[0]
        assert plan.n_voices == len(c.names) == len(upsampling_of(c))
        for v, name in enumerate(c.names):
            info = plan.voice_info(v)
            assert info.upsampling == upsampling_of(c)[v], (cell_id(c), name)
            d = oracle.derive(oracle_config(name, c.rate, c.delay, c.layout, c.precision))
            assert info.control_steps == d.control_steps and info.pad_size == d.pad_size, (cell_id(c), name)
            if name == "male":
                assert info.control_steps == TUBES[c.delay, c.layout]["steps"]
        steps = [int(plan.voice_info(v).control_steps) for v in range(plan.n_voices)]
        assert len(set(steps)) == len(steps), (cell_id(c), steps)  # every voice has its own internal rate
        pairs.add((tube_id(c.delay, c.layout), c.mix))
    assert len(pairs) == 15 and list(MIXES) == ["up", "mixed", "down"]


def test_launch_a_frame_counts_groups_and_copies():
    for c in LAUNCHABLE:
        plan, a = _case(c)
        chunk, rows = chunk_of(c), rows_of(c)
        assert chunk > 0 and chunk % 4 == 0 and rows == c.rows
        assert a.ids.size == batch_a(c) in (19, 30) and a.params.shape == (a.ids.size, max(int(a.frames.max()), 1), 16)
        assert np.bincount(a.ids).tolist() == utterances_per_voice(c) == [9, 10, 11][: len(c.names)], cell_id(c)
        assert (np.diff(a.ids) < 0).any()  # shuffled: the row map has work to do
        for v in range(len(c.names)):
            steps = int(plan.voice_info(v).control_steps)
            fa = a.pools[v][1]
            assert fa.size == POOL == len(set(fa.tolist())) and {0, 1, 2} <= set(fa.tolist()) and fa.max() <= MAX_FRAMES_A, (cell_id(c), v, fa)
            claimed = residues(steps, chunk)
            step = math.gcd(steps, chunk)
            # the shortest and the longest partial last chunk 48 frames reach, and a whole one where they reach one: on
            # male (voice 0) all three, 0, gcd and chunk - gcd
            assert claimed and (v > 0 or set(claimed) == {0, step % chunk, (chunk - step) % chunk}), (cell_id(c), v, claimed)
            for r in claimed:
                assert 0 <= r < chunk and [f for f in fa if f > 0 and (int(f) * steps) % chunk == r], (cell_id(c), v, r, fa)
            assert empty_rows(POOL + v, rows) == EMPTY_ROWS[rows][v], (cell_id(c), v)
            # the extra utterances: one more of each of the voice's v longest members
            times = np.bincount([t for (w, t) in a.member if w == v], minlength=POOL)
            longest = np.argsort(-fa, kind="stable")[:v]
            assert times.sum() == POOL + v and (times[longest] == 2).all() and (np.delete(times, longest) == 1).all(), (cell_id(c), v, times)
        for b, (v, t) in enumerate(a.member):
            f = int(a.pools[v][1][t])
            assert a.ids[b] == v and a.frames[b] == f and np.array_equal(a.params[b, :f], a.pools[v][0][t, :f]) and not a.params[b, f:].any()


def test_launch_b_has_no_utterance_of_voice_0_and_two_bad_ids():
    for c in LAUNCHABLE:
        n = len(c.names)
        b = launch_b(c, _case(c)[1])
        assert b.bad_ids.size == b.good_ids.size == b.frames.size == BATCH_B == b.params.shape[0]
        assert not (b.good_ids == 0).any() and ((b.good_ids >= 1) & (b.good_ids < n)).all() and set(range(1, n)) <= set(b.good_ids.tolist())
        bad = np.flatnonzero(b.bad_ids != b.good_ids)
        assert sorted(b.bad_ids[bad].tolist()) == [-1, n] and (b.frames > 0).all(), cell_id(c)


def test_output_counts_are_the_oracles_and_the_capacity_holds_them():
    for c in LAUNCHABLE:
        plan, a = _case(c)
        cfgs = [oracle_config(name, c.rate, c.delay, c.layout, c.precision) for name in c.names]
        b = launch_b(c, a)
        for ids, frames, width in ((a.ids, a.frames, a.params.shape[1]), (b.good_ids, b.frames, b.params.shape[1])):
            capacity = plan.voices_output_capacity(width)
            for v, f in zip(ids, frames):
                want = oracle.output_count(cfgs[int(v)], int(f))
                assert plan.voice_output_count(int(v), int(f)) == want <= capacity, (cell_id(c), int(v), int(f), want, capacity)


def test_no_two_utterances_of_launch_a_have_equal_expected_samples():
    """... unless one is a deliberate copy of the other: a row map that hands an utterance to the wrong row, or a workgroup
    on the wrong voice's constants, wavetable or ring, cannot pass the GPU test's comparison with the oracle.  (A 0-frame
    utterance is the converter's flush of silence: its zeros tell only voices with different counts apart.)"""
    for c in LAUNCHABLE:
        a = _case(c)[1]
        refs = oracle_pools(c, a)
        keys = sorted(refs)
        for k in keys:
            frames = int(a.pools[k[0]][1][k[1]])
            assert refs[k].any() == (frames > 0), (cell_id(c), k, frames)
        for k, m in itertools.combinations(keys, 2):
            if refs[k].any() or refs[m].any():
                assert not np.array_equal(refs[k], refs[m]), (cell_id(c), k, m)
        # and the utterances of launch B are members of these pools, every one with frames
        assert (launch_b(c, a).frames > 0).all()


def test_one_track_gives_different_samples_under_each_pair_of_voices():
    track = tracks.random_track(6, 4711, consonant_heavy=True)
    seen = set()
    for c in LAUNCHABLE:
        key = (c.precision == capi.PRECISION_F32, c.delay, c.layout, c.mix)
        if key in seen:
            continue
        seen.add(key)
        outs = oracle_many(c, [(v, track) for v in range(len(c.names))])
        for v, w in itertools.combinations(range(len(c.names)), 2):
            n = min(outs[v].size, outs[w].size)
            assert n > 0 and outs[v].any() and not np.array_equal(outs[v][:n], outs[w][:n]), (cell_id(c), v, w)
    assert len(seen) == 30
