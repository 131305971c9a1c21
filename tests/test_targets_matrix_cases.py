"""The case table of the targets matrix (targets_matrix_cases.py) held to design-only plans of the diagnostics library, to
the literal restatement of the rule and to the oracle's counts, so that what tests/test_gpu_targets_matrix.py runs on the
device is what its docstring says (CPU test).

    the split: the 79 / 11 of the one-shot launches and the 72 / 7 of the streams, as the hooks answer for plans at 250 Hz;
    every cell's C a positive multiple of 4, its N targets_cases.filter_length(internal rate);
    the pool: nine different step counts, the eight fixed ones, all four residues modulo 4, two lengths beyond N + C, the
    seeded one strictly between C and N;
    the lists: steps of edge_steps only, strictly increasing, 6 to 40 points but for the whole set, the point at step 0 and
    the empty list; finite values, positive on fricCF and fricBW;
    the cap on what may be left out is zero: in EVERY cell, one-shot and voices, the lists of the longest member reach
    EVERY coincidence (a) to (f) in EVERY tick group, so do the stream's lists, which also hold the steps around every
    resume of the session in every group, and every member's own lists reach (f);
    gvtm_targets_apply_host on every cell's lists equals targets_cases.apply_rule, the literal ring, for the pool members
    of up to N + C + 2 steps (the ring is slow; that passes every coincidence once);
    plan.targets_output_count is the oracle's count at one step per frame and targets_output_capacity holds it;
    no two pool members that are not copies have equal expected frames."""
import functools

import numpy as np

import oracle
import targets_cases
import voices_matrix_cases as vm
from gama_tts_amd import capi
from shape_matrix_cases import (BATCH, CELLS, FALL_BACK, LAUNCHABLE, POOL, STREAM_FALL_BACK, cell_id, chunk_length, float_model,
                                internal_rate, launch_shape, plan_of, seed_of, stream_launch_shape, stream_rows)
from targets_matrix_cases import (EMPTY, GROUPS, LETTERS, ONLY_STEP_0, STREAM_BATCH, VOICE_CELLS, WHOLE, coincidences, edge_lists,
                                  edge_steps, host_frames, pool_lists, resume_edges, slice_lists, step_pool, stream_bases, stream_pieces,
                                  stream_total, tiled_steps, voices_case)
from targets_cases import FRIC_BW, FRIC_CF

ALL = [LETTERS] * len(GROUPS)


def _design(cell, rows=None):
    return plan_of(cell, 250.0, capi.DEVICE_NONE, rows)


@functools.lru_cache(maxsize=None)
def _shapes():
    """(cell, C, N) of every launchable cell, from design-only plans."""
    out = []
    for c in LAUNCHABLE:
        plan = _design(c)
        out.append((c, chunk_length(plan), plan.targets_filter_length()))
        plan.close()
    return tuple(out)


def test_the_splits_are_the_shape_matrix_s():
    keeps = {cell_id(c) for c in CELLS if launch_shape(_design(c))[0] == c.rows}
    assert keeps == {cell_id(c) for c in LAUNCHABLE} and len(keeps) == 79 and len(CELLS) - len(keeps) == len(FALL_BACK) == 11
    falls = {cell_id(c) for c in LAUNCHABLE if stream_launch_shape(_design(c), STREAM_BATCH)[0] != c.rows}
    assert falls == STREAM_FALL_BACK and len(falls) == 7 and len(LAUNCHABLE) - len(falls) == 72
    for c in LAUNCHABLE:
        assert stream_launch_shape(_design(c), STREAM_BATCH)[0] == stream_rows(c), cell_id(c)
    assert len(VOICE_CELLS) == 34 and {c.mix for c in VOICE_CELLS} == {"mixed"} and all(c.names == ("male", "female", "baby") for c in VOICE_CELLS)
    assert {vm.cell_id(c) for c in vm.CELLS if c.mix == "mixed"} - {vm.cell_id(c) for c in VOICE_CELLS} == {i for i in vm.VOICES_FALL_BACK if "-mixed-" in i}


def test_chunk_and_filter_length_of_every_cell():
    for c, C, N in _shapes():
        assert C > 0 and C % 4 == 0, (cell_id(c), C)
        assert N == targets_cases.filter_length(_design(c).info.internal_rate_hz) > 2 * C, (cell_id(c), N)
        assert abs(N - 0.05 * internal_rate(c)) <= 1.0, (cell_id(c), N)
    assert len({(C, N) for _, C, N in _shapes()}) >= 15  # (the same lists meet a chunk edge elsewhere from shape to shape)


def test_pool_of_every_cell():
    for c, C, N in _shapes():
        pool = step_pool(C, N, seed_of(c))
        assert pool.size == POOL == len(set(pool.tolist())), (cell_id(c), pool)
        assert pool[:8].tolist() == [0, 1, C - 1, C, 2 * C + 1, N - 1, N + C + 2, 2 * N + 3] and C < pool[8] < N, (cell_id(c), pool)
        assert {int(s) % 4 for s in pool} == {0, 1, 2, 3} and (pool > N + C).sum() >= 1 and pool.max() == 2 * N + 3, (cell_id(c), pool)
        steps, idx = tiled_steps(pool)
        assert steps.size == BATCH and all((idx == t).sum() >= 2 and steps[idx == t].tolist() == [pool[t]] * int((idx == t).sum()) for t in range(POOL))
        total, pieces = stream_total(C, N), stream_pieces(C, N)
        assert sum(pieces) == total == N + 3 * C + 70 and pieces[-1] == 33 and pieces[:3] == [1, 11, 13] and min(pieces) > 0


def _check_lists(lists, C, N, S, what, extra=()):
    allowed = set(edge_steps(C, N, S, extra).tolist())
    assert len(lists) == 16
    for p, (steps, values) in enumerate(lists):
        assert len(steps) == len(values) and values.dtype == np.float32 and np.isfinite(values).all(), (what, p)
        assert set(steps) <= allowed and all(b > a for a, b in zip(steps, steps[1:])), (what, p)
        if p in (FRIC_CF, FRIC_BW):
            assert (values > 0.0).all() and steps[0] == 0, (what, p)
        if p >= 7 and p != EMPTY:
            assert steps[0] == 0, (what, p)  # no radius starts at 0
        if p not in (WHOLE, ONLY_STEP_0, EMPTY):
            assert min(6, len(allowed) - 4) <= len(steps) <= 41 + len(extra), (what, p, len(steps))
    assert lists[EMPTY][0] == [] and lists[ONLY_STEP_0][0] == [0] and lists[WHOLE][0] == sorted(allowed)
    if S >= N + C:
        assert len(lists[WHOLE][0]) > 64, what
    if S >= 2 * N:
        assert targets_cases.status_of(S, lists) == 0


def test_lists_and_coincidences_of_every_cell():
    """No cell and no coincidence is left out."""
    for c, C, N in _shapes():
        pool = step_pool(C, N, seed_of(c))
        lists = pool_lists(C, N, pool, seed_of(c))
        for t in range(POOL):
            S = int(pool[t])
            _check_lists(lists[t], C, N, S, (cell_id(c), S))
            reached = coincidences(lists[t], C, N, S)
            assert all("f" in r for r in reached), (cell_id(c), S, reached)
            if S == pool.max():
                assert reached == ALL, (cell_id(c), S, reached)
        total, pieces = stream_total(C, N), stream_pieces(C, N)
        bases = stream_bases(pieces)
        # (launches of whole granules: the resumes are not where the pieces end; one falls behind the window)
        assert len(bases) >= 5 and all(b % 12 == 0 for b in bases) and bases[:2] == [12, 24] and max(bases) > N and set(bases) - set(np.cumsum(pieces).tolist())
        extra = resume_edges(bases, N)
        assert {s for b in bases for s in (b - 1, b)} <= set(extra) and {b - 1 - N for b in bases if b > N + 1} <= set(extra)
        for b in range(STREAM_BATCH):
            stream = edge_lists(C, N, total, seed_of(c) + 50 + b, extra)
            _check_lists(stream, C, N, total, (cell_id(c), "stream", b), extra)
            assert coincidences(stream, C, N, total) == ALL, (cell_id(c), "stream", b)
            assert all(any(set(extra) <= set(stream[p][0]) for p in group) for group in GROUPS), (cell_id(c), "stream", b)


def test_coincidences_sees_what_is_missing():
    """The function that both tests trust, on lists written by hand: C 8, N 21, S 60."""
    C, N, S = 8, 21, 60
    none = [([], np.zeros(0, np.float32))] * 16

    def group0(steps):
        return coincidences([(steps, np.zeros(len(steps), np.float32))] + none[1:], C, N, S)

    assert group0([]) == ["", "", ""] and group0([0, 8]) == ["", "", ""] and group0([8, 15]) == ["a", "", ""]
    assert group0([0, 21 + 8]) == ["", "", ""]  # (the point at step 0 never leaves)
    # (a point in the block the leave move lands in: no longer b, and with it d)
    assert group0([11, 18]) == ["b", "", ""] and group0([11, 18, 33]) == ["d", "", ""] and group0([11, 18, 44]) == ["b", "", ""]
    assert group0([11, 32]) == ["c", "", ""] and group0([11, 33]) == ["d", "", ""] and group0([11, 36]) == ["", "", ""]
    assert group0([41, 42, 43]) == ["e", "", ""] and group0([41, 42, 44]) == ["", "", ""]
    assert group0([59, 60, 61]) == ["f", "", ""] and group0([60, 61]) == ["", "", ""]
    assert group0([59 - 21, 59]) == ["c", "", ""] and group0([60 - 21, 60]) == ["", "", ""]  # a move counts inside the S steps only
    spread = list(none)
    spread[3], spread[6] = ([8], np.zeros(1, np.float32)), ([15], np.zeros(1, np.float32))
    assert coincidences(spread, C, N, S) == ["", "a", ""]  # (one parameter of the group each)


def test_the_voices_cases_reach_every_coincidence_under_every_voice_s_own_n():
    for cell in VOICE_CELLS:
        plan = vm.voices_plan(cell, capi.DEVICE_NONE)
        C = vm.chunk_of(cell)
        n = [plan.targets_filter_length(v) for v in range(3)]
        assert len(set(n)) == 3 and vm.voices_launch_shape(plan, 20)[0] == cell.rows, vm.cell_id(cell)
        case = voices_case(cell, plan)
        assert len(case.step_counts) == 20 and case.voice_ids[case.bad] == 3 and sorted(case.voice_ids) == [0] * 7 + [1] * 6 + [2] * 6 + [3]
        assert case.voice_ids[: case.bad] + case.voice_ids[case.bad + 1:] != sorted(case.voice_ids[: case.bad] + case.voice_ids[case.bad + 1:])
        for v in range(3):
            mine = [b for b, w in enumerate(case.voice_ids) if w == v]
            assert {0, C, 2 * C + 1, n[v] - 1, n[v] + C + 2, 2 * n[v] + 3} <= {case.step_counts[b] for b in mine}, (vm.cell_id(cell), v)
            longest = max(mine, key=lambda b: case.step_counts[b])
            assert coincidences(case.utterances[longest], C, n[v], 2 * n[v] + 3) == ALL, (vm.cell_id(cell), v)
            for b in mine:
                _check_lists(case.utterances[b], C, n[v], case.step_counts[b], (vm.cell_id(cell), b))
                assert plan.targets_voice_output_count(v, case.step_counts[b]) <= plan.targets_voices_output_capacity(max(case.step_counts))
        plan.close()


def test_host_rule_equals_the_literal_ring_on_every_cell_s_lists():
    for c, C, N in _shapes():
        plan = _design(c)
        pool = step_pool(C, N, seed_of(c))
        lists = pool_lists(C, N, pool, seed_of(c))
        for t in range(POOL):
            S = int(pool[t])
            if S > N + C + 2:
                continue
            want, status = targets_cases.apply_rule(lists[t], S, N)
            assert status == 0
            got = host_frames(plan, lists[t], S)
            assert got.shape == want.shape and got.tobytes() == want.tobytes(), (cell_id(c), S)
        plan.close()


def test_counts_capacity_and_frames_that_differ():
    for c, C, N in _shapes():
        plan = _design(c)
        rate = plan.info.internal_rate_hz
        cfg = oracle.male_config(c.rate, c.delay, c.layout, float_model=float_model(c))
        assert oracle.derive(cfg, rate).control_steps == 1, cell_id(c)
        pool = step_pool(C, N, seed_of(c))
        capacity = plan.targets_output_capacity(int(pool.max()))
        for S in list(pool) + [stream_total(C, N)]:
            want = oracle.output_count(cfg, int(S), rate)
            assert plan.targets_output_count(int(S)) == want <= capacity, (cell_id(c), int(S), want, capacity)
        lists = pool_lists(C, N, pool, seed_of(c))
        frames = [host_frames(plan, lists[t], int(pool[t])) for t in range(POOL)]
        for t in range(POOL):
            for s in range(t):
                m = int(min(pool[s], pool[t]))
                assert m == 0 or not np.array_equal(frames[s][:m], frames[t][:m]), (cell_id(c), s, t)
        plan.close()


def test_slice_lists_cuts_a_session_into_its_pushes():
    C, N = 48, 1002
    total, lists = stream_total(C, N), edge_lists(48, 1002, stream_total(48, 1002), 3)
    done, seen = 0, [[] for _ in range(16)]
    for piece in stream_pieces(C, N):
        for p, (steps, values) in enumerate(slice_lists(lists, done, piece)):
            assert all(0 <= s < piece for s in steps) and len(steps) == len(values)
            seen[p] += [(s + done, float(v)) for s, v in zip(steps, values)]
        done += piece
    assert done == total
    for p in range(16):
        assert seen[p] == [(s, float(v)) for s, v in zip(*lists[p]) if s < total], p
