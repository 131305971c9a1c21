"""Streams fed parameter targets on model 5 plans (gvtm_stream_push_targets_model5), the host side.  No GPU needed.

Pins: the name in the header, the library and the binding, with gvtm_stream_push_targets' prototype argument for argument;
the refusal of a null stream; the rule from any step (gvtm_targets_apply_host_from, the text the kernel's interpolation lanes
resume on) at model 5's filter length N = 3021 under the cuts a granule of FOUR steps makes -- piece by piece it gives the
frames and the sums of the whole, on design-only model 5 plans of both classes, over stream_targets5_cases.pieces5 for the four
chunks of the kernel's targets variant and over the edge session; and the edge lists' own sanity: every claimed edge is where
it says, and the host rule's frames keep r1..r8, fricCF and fricBW above 0 at every step, so that the GPU tests never depend
on what the model does with a closed tube."""
import subprocess

import numpy as np
import pytest

import gama_tts_amd as g
from gama_tts_amd import capi
import stream_targets5_cases as sessions5
import targets5_cases as cases
from test_capi_prototypes_cpu import HEADER, c_prototypes, problems, read
from voice_cases import model5_plan

INVALID_ARGUMENT = 1
ENTRY = "gvtm_stream_push_targets_model5"
N = cases.N
EDGE_TOTAL = 3 * N + 45


@pytest.fixture(scope="module")
def plans():
    return {float_class: model5_plan(device=capi.DEVICE_NONE, float_class=float_class) for float_class in (True, False)}


def test_the_name_in_the_header_the_library_and_the_binding():
    out = subprocess.run(["nm", "-D", "--defined-only", capi.library_path()], check=True, capture_output=True, text=True).stdout
    assert ENTRY in {line.split()[-1] for line in out.splitlines() if line.split()}
    header = c_prototypes(read(HEADER))
    assert ENTRY in header and ENTRY in capi.PROTOTYPES
    assert problems({ENTRY: header[ENTRY]}, {ENTRY: capi.PROTOTYPES[ENTRY]}) == []
    # argument for argument gvtm_stream_push_targets'
    assert header[ENTRY] == header["gvtm_stream_push_targets"]
    assert capi.PROTOTYPES[ENTRY] == capi.PROTOTYPES["gvtm_stream_push_targets"]
    assert callable(getattr(capi.Stream, "push_targets_model5"))


def test_a_null_stream_is_refused():
    lib = g.load_library()
    assert getattr(lib, ENTRY)(None, capi._ptr(np.zeros(17, np.int64)), None, None, None, 0, None, 0, None, None) == INVALID_ARGUMENT
    assert b"null stream" in lib.gvtm_last_error()


def whole(plan, lists, total):
    frames, status = capi.targets_apply_host(plan, lists, total)
    assert status == 0
    _, sums, status = capi.targets_apply_host_from(plan, lists, 0, total, np.full(16, 123.0))  # (from 0 the sums on input are not read)
    assert status == 0
    return frames, sums


def in_pieces(plan, lists, pieces):
    frames, sums, first = [], np.zeros(16), 0
    for count in pieces:
        out, sums, status = capi.targets_apply_host_from(plan, lists, first, count, sums)
        assert status == 0, first
        frames.append(out)
        first += count
    return np.concatenate(frames), sums


def granule_cuts(pieces):
    """What the stream makes of the pieces: every push synthesizes up to the last multiple of four it has been given."""
    cuts, given, done = [], 0, 0
    for p in pieces:
        given += p
        upto = given // sessions5.GRANULE * sessions5.GRANULE
        if upto > done:
            cuts.append(upto - done)
            done = upto
    return cuts + ([given - done] if given > done else [])  # (finish: the pending steps)


def sessions_of():
    """(name, lists, total, pieces) of every session the resume is held to."""
    for float_class in (True, False):
        for chunk in cases.CHUNKS[float_class]:
            total = 2 * N + chunk + 5
            yield "pieces5-%d" % chunk, cases.lists_of(total), total, sessions5.pieces5(chunk, N)
    yield "edges", sessions5.edge_lists5(N, EDGE_TOTAL), EDGE_TOTAL, sessions5.edge_pieces5(N, EDGE_TOTAL)
    for chunk in sorted(set(cases.CHUNKS[True] + cases.CHUNKS[False])):
        yield "edges-at-chunk-%d" % chunk, sessions5.edge_lists5(N, EDGE_TOTAL), EDGE_TOTAL, sessions5.edge_pieces5_at_chunk(chunk, N, EDGE_TOTAL)


@pytest.mark.parametrize("float_class", [True, False], ids=["float", "double"])
def test_resume_at_the_granule_of_four_equals_the_whole(plans, float_class):
    plan = plans[float_class]
    assert plan.targets_filter_length() == N
    seen = 0
    for name, lists, total, pieces in sessions_of():
        assert sum(pieces) == total, name
        want, want_sums = whole(plan, lists, total)
        # as pushed, and as the stream launches them
        for cuts in (pieces, granule_cuts(pieces)):
            assert sum(cuts) == total and (cuts is pieces or all(c % 4 == 0 for c in cuts[:-1])), name
            got, sums = in_pieces(plan, lists, cuts)
            assert got.shape == want.shape and got.tobytes() == want.tobytes(), name
            assert sums.tobytes() == want_sums.tobytes(), name
        seen += 1
    assert seen == 4 + 1 + 4


def test_the_sessions_cover_what_they_claim(plans):
    for chunk in (60, 52, 56, 24):
        assert sessions5.pieces5(chunk, N) == [1, 3, 4, 5, chunk - 1, chunk, chunk + 1, N - 1, N - 2 * chunk - 7]
    total = EDGE_TOTAL
    assert sessions5.edge_pieces5(N, total) == [1, 3, 4, 5, N - 1, N, N + 1, 32]
    b = sessions5.edge_boundaries5(N, total)
    assert b == [0, 1, 4, 8, 13, N + 12, 2 * N + 12, 3 * N + 13]
    for chunk in (60, 52, 56, 24):
        refined = sessions5.edge_pieces5_at_chunk(chunk, N, total)
        starts = set(np.cumsum([0] + refined)[:-1].tolist())
        assert sum(refined) == total and set(b) <= starts and {chunk - 1, chunk, chunk + 1} <= starts
        assert N in refined and N + 1 in refined
    lists = sessions5.edge_lists5(N, total)
    steps = [l[0] for l in lists]
    assert all(len(l[0]) == len(l[1]) and l[1].dtype == np.float32 for l in lists)
    assert all(all(0 <= s < total for s in st) and all(y > x for x, y in zip(st, st[1:])) for st in steps)
    # the two kinds without a point at step 0, on aspVol, fricVol and velum alone
    late = [p for p in range(16) if not steps[p] or steps[p][0] > 0]
    assert sorted(late) == [sessions5.ASP_VOL, sessions5.FRIC_VOL, sessions5.VELUM]
    assert steps[sessions5.ASP_VOL] == [] and steps[sessions5.FRIC_VOL] == [b[7], total - 1] and steps[sessions5.VELUM][0] == b[5]
    assert all(lists[p][1][0] > 0 for p in (sessions5.FRIC_VOL, sessions5.VELUM))  # (a late start that is heard)
    assert steps[4] == [0]
    # points at a piece's first and last step, and exactly N before a boundary
    assert set(steps[1][1:]) <= set(b) and {s + 1 for s in steps[7][1:]} <= set(b) and len(steps[1]) == len(steps[7]) == 4
    assert {s + N for s in steps[8][1:]} == {b[5], b[6], b[7]} and min(steps[8][1:]) > 0
    assert steps[10][1:] == [b[5] - N - 1, b[5] - N, b[5] - N + 1]
    # thirty points inside one window, behind a boundary
    assert len(steps[0]) == 31 and steps[0][-1] - steps[0][1] < N and b[5] <= steps[0][1] < b[5] + 4
    # around the granule's multiples
    assert steps[11] == [0, 3, 4, 5, 7, 8, 9]
    # wide values on fricCF and fricBW only, positive, six decades apart within one window
    for p in (cases.targets_cases.FRIC_CF, cases.targets_cases.FRIC_BW):
        values = lists[p][1].astype(np.float64)
        assert (values > 0).all() and values.min() < 1e-2 and values.max() > 1e3
        assert max(np.diff(steps[p])) < N
    for p in set(range(16)) - {cases.targets_cases.FRIC_CF, cases.targets_cases.FRIC_BW}:
        assert len(lists[p][1]) == 0 or np.abs(lists[p][1]).max() < 100.0
    # what model 5 is fed: open radii and positive band-pass frequencies at every step, in both classes
    for float_class in (True, False):
        frames, status = capi.targets_apply_host(plans[float_class], lists, total)
        assert status == 0 and frames.shape == (total, 16) and np.isfinite(frames).all()
        assert (frames[:, list(sessions5.RADII)] > 0).all()
        assert (frames[:, 5] > 0).all() and (frames[:, 6] > 0).all()
        assert (frames[:, [sessions5.ASP_VOL, sessions5.FRIC_VOL, sessions5.VELUM]] >= 0).all()
        assert (frames[: b[7], sessions5.FRIC_VOL] == 0).all() and frames[-1, sessions5.FRIC_VOL] > 0
