"""The rule of the parameter targets from any step (gvtm_targets_apply_host_from; csrc/vtm_targets.hpp: targets_resume, the one
text the synthesis kernel's interpolation lanes run on behalf of a stream) and the refusals of the targets-fed streams'
entries that need no device.  No GPU needed.

Pins: a session cut into pieces (stream_targets_cases.pieces: around the granule of 12 steps and around the window), the sums
carried from piece to piece, gives byte for byte the frames of one gvtm_targets_apply_host call and the sums of one call
from 0 -- on every case of targets_cases.CASES, on seeded random lists and on lists written for the edges of resuming; the
same with the lists trimmed before every piece by the literal restatement of what a list may forget, and NOT the same
with one point more forgotten; the statuses and refusals of the entry; the names in the header, the library and the
binding."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import gama_tts_amd as g
from gama_tts_amd import capi
import stream_targets_cases as sessions
import targets_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARGUMENT = 0, 1
ENTRIES = ("gvtm_targets_apply_host_from", "gvtm_stream_push_targets", "gvtm_stream_targets_capacity", "gvtm_stream_targets_points")


@pytest.fixture(scope="module")
def plans():
    return {key: cases.make_plan(key, capi.DEVICE_NONE) for key in cases.RULE_PLANS}


def in_pieces(plan, lists, total, n, trim=None):
    """The session piece by piece -> (frames float32 [total][16], the sums after the last step).  trim(lists, s0, n): what
    the lists are cut down to before the piece that begins at step s0."""
    frames, sums, first = [], np.zeros(16), 0
    for count in sessions.pieces(n, total) or [0]:  # (a session of no steps: one call for its sums)
        given = lists if trim is None else trim(lists, first, n)
        out, sums, status = capi.targets_apply_host_from(plan, given, first, count, sums)
        assert status == 0, first
        frames.append(out)
        first += count
    assert first == total
    return (np.concatenate(frames) if frames else np.zeros((0, 16), np.float32)), sums


def whole(plan, lists, total):
    frames, status = capi.targets_apply_host(plan, lists, total)
    assert status == 0
    _, sums, status = capi.targets_apply_host_from(plan, lists, 0, total, np.full(16, 123.0))  # (from 0 the sums on input are not read)
    assert status == 0
    return frames, sums


def sessions_of(plans):
    """(name, plan, n, total, lists) of every session the resume is held to."""
    for name in cases.CASES:
        key, total, lists = cases.case(name)
        yield name, plans[key], cases.filter_length(cases.PLANS[key].rate), total, lists
    for key in cases.RULE_PLANS:
        n = cases.filter_length(cases.PLANS[key].rate)
        total = 4 * n + 50
        yield key + "-edges", plans[key], n, total, sessions.edge_lists(n, total)
    n = cases.filter_length(cases.PLANS["male"].rate)
    for seed in range(12):
        total = (3 * n + 37 + 5, 4 * n + 50, 2 * n + 36, n + 40)[seed % 4]
        yield "random-%d" % seed, plans["male"], n, total, sessions.random_lists(n, total, seed)


def test_names_in_the_header_the_library_and_the_binding():
    header = open(os.path.join(ROOT, "include", "gama_vtm.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", capi.library_path()], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    for name in ENTRIES:
        assert name + "(" in header and name in exported and name in capi.PROTOTYPES, name
    assert all(callable(getattr(capi.Stream, name)) for name in ("push_targets", "targets_capacity", "targets_points"))
    assert callable(capi.targets_apply_host_from)


def test_the_sessions_cover_what_they_claim():
    n = cases.filter_length(cases.PLANS["male"].rate)
    total = 4 * n + 50
    assert sessions.pieces(n, total) == [1, 11, 12, 13, n - 1, n, n + 1, total - 3 * n - 37]
    assert sessions.pieces(n, 20) == [1, 11, 8] and sessions.pieces(n, 0) == [] and sessions.pieces(n, 12) == [1, 11]
    b = sessions.boundaries(n, total)
    lists = sessions.edge_lists(n, total)
    steps = [l[0] for l in lists]
    assert steps[0] == [0] and steps[1] == []
    assert set(steps[2]) <= set(b) and {s + 1 for s in steps[3]} <= set(b)
    assert {s + n for s in steps[4]} <= set(b) and min(steps[4]) > 0
    for p in (cases.FRIC_CF, cases.FRIC_BW):  # wide values: six decades apart within one window
        mags = np.abs(lists[p][1].astype(np.float64))
        assert mags.min() < 1e-5 and mags.max() > 1e3
    assert len(steps[7]) == 30 and steps[7][-1] - steps[7][0] < n and any(b_ <= steps[7][0] < b_ + 4 for b_ in b)
    # the restated forgetting: the last point at or before the far edge stays, with everything after it
    some = [([0, 5, 9, 30], np.float32([1, 2, 3, 4]))]
    assert sessions.forget(some, 10 + n, n)[0][0] == [9, 30] and sessions.forget(some, 9 + n, n)[0][0] == [5, 9, 30]
    assert sessions.forget(some, n, n)[0][0] == [0, 5, 9, 30] and sessions.forget(some, 31 + n, n)[0][0] == [30]
    assert sessions.forget(some, 10 + n, n, one_more=True)[0][0] == [30] and sessions.forget(some, n, n, one_more=True)[0][0] == [0, 5, 9, 30]


def test_resume_equals_the_whole(plans):
    seen = 0
    for name, plan, n, total, lists in sessions_of(plans):
        want, want_sums = whole(plan, lists, total)
        got, sums = in_pieces(plan, lists, total, n)
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), name
        assert sums.tobytes() == want_sums.tobytes(), name
        seen += 1
    assert seen >= len(cases.CASES) + 15


def test_the_sum_is_carried_because_it_cannot_be_recomputed(plans):
    """On the wide lists the carried sum is not the sum of the window's values: resuming on that one gives other bytes."""
    n = cases.filter_length(cases.PLANS["male"].rate)
    total = 4 * n + 50
    lists = sessions.edge_lists(n, total)
    want, _ = whole(plans["male"], lists, total)
    first = 2 * n + 36
    fed = np.zeros(total, np.float64)
    steps, values = lists[cases.FRIC_CF]
    for s, v in zip(steps, values):
        fed[s:] = float(v)
    _, sums, _ = capi.targets_apply_host_from(plans["male"], lists, 0, first, np.zeros(16))
    exact = float(np.sum([np.float64(v) for v in fed[first - n:first]]))
    assert exact != sums[cases.FRIC_CF]
    doctored = sums.copy()
    doctored[cases.FRIC_CF] = exact
    rest, _, status = capi.targets_apply_host_from(plans["male"], lists, first, total - first, doctored)
    assert status == 0 and rest[:, cases.FRIC_CF].tobytes() != want[first:, cases.FRIC_CF].tobytes()
    others = [p for p in range(16) if p != cases.FRIC_CF]
    assert rest[:, others].tobytes() == want[first:, others].tobytes()


def test_forgetting_by_the_rule_gives_the_same_bytes(plans):
    dropped = 0
    for name, plan, n, total, lists in sessions_of(plans):
        want, want_sums = whole(plan, lists, total)
        got, sums = in_pieces(plan, lists, total, n, trim=sessions.forget)
        assert got.tobytes() == want.tobytes() and sums.tobytes() == want_sums.tobytes(), name
        last = sessions.boundaries(n, total)[-1] if total else 0
        dropped += sum(len(l[0]) for l in lists) - sum(len(l[0]) for l in sessions.forget(lists, last, n))
    assert dropped > 200  # (the sessions are long enough for the rule to forget most of their points)


def test_forgetting_one_point_more_is_told(plans):
    n = cases.filter_length(cases.PLANS["male"].rate)
    total = 4 * n + 50
    lists = sessions.edge_lists(n, total)
    want, _ = whole(plans["male"], lists, total)
    got, _ = in_pieces(plans["male"], lists, total, n, trim=lambda l, s0, n_: sessions.forget(l, s0, n_, one_more=True))
    p = sessions.FORGET
    assert got[:, p].tobytes() != want[:, p].tobytes()
    # ... from the piece on whose far edge has passed the point at step 20: in front of it nothing is missed
    first_missed = sessions.boundaries(n, total)[5]
    assert first_missed - 1 - n >= 20 and got[:first_missed, p].tobytes() == want[:first_missed, p].tobytes()
    assert got[first_missed, p] != want[first_missed, p]


# ---- statuses and refusals ----

def call_from(plan, lists, first_step, n_steps, offsets=None, guard=-3.25):
    table, steps, values = capi.pack_targets(lists)
    if offsets is not None:
        table = np.asarray(offsets, dtype=np.int64)
    out = np.full((max(n_steps, 1) if 0 <= n_steps < 10 ** 6 else 1, 16), guard, dtype=np.float32)
    sums = np.full(16, 9.0)
    status = ctypes.c_int32(-5)
    rc = plan._lib.gvtm_targets_apply_host_from(plan._h, 0, capi._ptr(table), capi._ptr(steps), capi._ptr(values), int(first_step), int(n_steps),
                                                capi._ptr(sums), capi._ptr(out), ctypes.byref(status))
    assert rc == OK
    return out, sums, int(status.value)


def test_statuses_of_the_entry(plans):
    plan = plans["male"]
    good = [([0, 3], np.float32([1.0, 2.0]))] + [([], np.float32([]))] * 15
    with_list = lambda p, steps, values: good[:p] + [(steps, np.float32(values))] + good[p + 1:]  # noqa: E731
    table = [0, 2] + [2] * 15
    limit = cases.STEP_LIMIT
    for first, n_steps, lists, offsets, want in [
            (0, 5, good, None, 0), (7, 5, good, None, 0), (7, 0, good, None, 0),
            (-1, 5, good, None, 1), (-1, 0, good, None, 1), (7, -1, good, None, 1),
            (limit - 5, 5, good, None, 1), (limit, 0, good, None, 1), (5, limit - 5, good, None, 1), (2 ** 62, 2 ** 62, good, None, 1),
            (-1, 5, good, [0, 2, 1] + [2] * 14, 1),                                       # 1 before 2
            (7, 5, good, [0, 2, 1] + [2] * 14, 2), (7, 5, good, [-1] + table[1:], 2),
            (7, 5, with_list(3, [1], [np.nan]), None, 3), (7, 5, with_list(15, [1], [np.inf]), None, 3),
            (7, 5, with_list(1, [4, 4], [1.0, 2.0])[:15] + [([2], np.float32([np.nan]))], None, 3),  # 3 before 4
            (7, 5, with_list(1, [-1], [1.0]), None, 4), (7, 5, with_list(7, [4, 9, 8], [1.0, 2.0, 3.0]), None, 4)]:
        out, sums, status = call_from(plan, lists, first, n_steps, offsets)
        assert status == want, (first, n_steps, offsets)
        if want:
            assert (out == -3.25).all() and (sums == 9.0).all()  # a refused utterance leaves its outputs alone
    # the last steps the counter holds are synthesized
    out, _, status = call_from(plan, good, limit - 6, 5)
    assert status == 0 and (out[:5] != -3.25).all()


def test_bad_calls_of_the_entry(plans):
    lib, plan, p = g.load_library(), plans["male"], capi._ptr
    offsets, steps, values = capi.pack_targets([([0], [1.0])] + [([], [])] * 15)
    out, sums = np.zeros((4, 16), np.float32), np.zeros(16)
    status = ctypes.c_int32(-5)

    def call(plan_h=plan._h, voice=0, offsets=offsets, steps=steps, values=values, first=3, n_steps=4, sums=sums, out=out, status=status):
        return lib.gvtm_targets_apply_host_from(plan_h, voice, p(offsets), p(steps), p(values), first, n_steps, p(sums), p(out),
                                                ctypes.byref(status) if status is not None else None)

    assert call() == OK and status.value == 0
    for bad in (dict(plan_h=None), dict(status=None), dict(offsets=None), dict(sums=None), dict(out=None), dict(steps=None), dict(values=None),
                dict(voice=1), dict(voice=-1), dict(sums=None, first=0)):
        status.value = -5
        assert call(**bad) == INVALID_ARGUMENT and status.value == -5, bad
        assert lib.gvtm_last_error()
    assert call(offsets=np.zeros(17, np.int64), steps=None, values=None) == OK and status.value == 0
    assert call(out=None, n_steps=0) == OK and status.value == 0


def test_the_stream_entries_refuse_a_null_stream():
    lib = g.load_library()
    held = np.zeros(4, np.int64)
    assert lib.gvtm_stream_push_targets(None, capi._ptr(np.zeros(17, np.int64)), None, None, None, 0, None, 0, None, None) == INVALID_ARGUMENT
    assert b"null stream" in lib.gvtm_last_error()
    assert lib.gvtm_stream_targets_capacity(None, 5) == ctypes.c_size_t(-1).value
    assert lib.gvtm_stream_targets_points(None, capi._ptr(held)) == INVALID_ARGUMENT
