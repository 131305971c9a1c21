"""Intonation contours applied to event lists, on the host: gvtm_intonation_apply_host against the reference's own
clearMacroIntonation() + prepareMacroIntonationInterpolation() (tests/golden/intonation_golden.npz), its statuses and bad
calls, the restatement of tests/intonation_cases.py on fresh random cases, and the device entries' checks as far as a
design-only plan lets them go.  No GPU needed."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import gama_tts_amd as g
from gama_tts_amd import capi
import event_lists
import intonation_cases as cases
from track_cases import product_config
from voice_cases import configs, male_plan, track_configs

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OK, INVALID_ARGUMENT, NO_DEVICE = 0, 1, 2
ENTRIES = ("gvtm_intonation_apply_host", "gvtm_apply_intonation_device", "gvtm_synthesize_intonation_device")


@pytest.fixture(scope="module")
def fixture():
    z = np.load(os.path.join(HERE, "golden", "intonation_golden.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def base_tables(golden_tracks):
    return cases.bases(golden_tracks)


def apply_host(cfg, table, points, **kw):
    return capi.intonation_apply_host(cfg, capi.events_from_table(table), capi.points_from_table(points), **kw)


def raw_apply(cfg, events, n_events, points, n_points, out, capacity, status=True):
    """The C entry as it is, nulls and all -> (return value, status)."""
    lib = g.load_library()
    st = ctypes.c_int32(-9)
    n = lib.gvtm_intonation_apply_host(ctypes.byref(cfg) if cfg is not None else None, capi._ptr(events), n_events, capi._ptr(points), n_points,
                                       capi._ptr(out), capacity, ctypes.byref(st) if status else None)
    return n, st.value


def test_cases_cover_what_they_claim(base_tables):
    """The generator's cases still are what the fixture was made from, and reach the placements their names say."""
    seen = {"on": 0, "new": 0, "behind": 0, "end": 0, "negative": 0, "front": 0}
    for name in cases.CASES:
        table, points, c = cases.case(name, base_tables)
        cp, times = int(c[0]), table[:, 0]
        for t in points[:, 0]:
            q = cases.point_time(float(t), cp, int(times[-1]))
            seen["on" if q in times else "new"] += 1
            seen["behind"] += q > times[-1]
            seen["end"] += t == times[-1] + 100 + cp
            seen["negative"] += t < 0
            seen["front"] += q < times[0]
    assert all(seen.values()), seen
    assert {c[3] for c in cases.CASES.values()} >= {0, 1, 2, 12, 64}
    assert {(c[1], c[2]) for c in cases.CASES.values()} >= {(cp, s) for cp in (1, 2, 3, 4) for s in (0, 1)}


@pytest.mark.parametrize("name", list(cases.CASES))
def test_host_entry_is_the_references_list(fixture, base_tables, name):
    table, points, c = cases.case(name, base_tables)
    assert cases.sha256(table, "<f8") == bytes(fixture[name + "__base_sha256"]).decode(), "the base list is not the fixture's any more"
    assert cases.sha256(points, "<f8") == bytes(fixture[name + "__points_sha256"]).decode(), "the points are not the fixture's any more"
    cfg = product_config(c)
    merged, status = apply_host(cfg, table, points)
    assert status == 0
    assert cases.check_merged(fixture, name, cases.events_to_table(merged)) is None
    # the frames generateOutput() then yields
    assert capi.tracks_frame_count(cfg, merged) == int(fixture[name + "__count"])
    # count-only mode, and an output of exactly the merged length
    assert apply_host(cfg, table, points, count_only=True) == (merged.shape[0], 0)
    exact, status = apply_host(cfg, table, points, capacity=merged.shape[0])
    assert status == 0 and exact.tobytes() == merged.tobytes()
    # base events keep every bit outside has_interp and interp
    kept = merged[np.isin(merged["time_ms"], table[:, 0].astype(np.int32))]
    base = capi.events_from_table(table)
    assert kept["param"].tobytes() == base["param"].tobytes() and kept["special"].tobytes() == base["special"].tobytes()


def test_base_events_keep_nan_payloads_and_lose_their_polynomials():
    """Rule 1 with P = 0: a copy bit for bit (a signalling NaN's payload included), has_interp and interp cleared."""
    base = capi.events_from_table(event_lists.random_event_table(5, n_events=6))
    base["has_interp"] = 1
    base["interp"] = 3.5
    base["param"][2, 3:5] = np.array([0x7FF0000000000001, 0xFFF8DEADBEEF0001], dtype=np.uint64).view(np.float64)
    merged, status = capi.intonation_apply_host(product_config(cases.cfg()), base, np.zeros(0, capi.POINT_DTYPE))
    assert status == 0 and merged.shape == base.shape
    assert merged["param"].tobytes() == base["param"].tobytes() and merged["special"].tobytes() == base["special"].tobytes()
    assert np.array_equal(merged["time_ms"], base["time_ms"])
    assert not merged["has_interp"].any() and not merged["interp"].any()


def test_every_status_from_its_smallest_input():
    cfg = product_config(cases.cfg(4))
    one = event_lists.random_event_table(1, n_events=1)                      # duration 100: points up to 104
    pts = lambda *times: np.array([[t, 1.0, 0.0] for t in times])            # noqa: E731
    empty = np.zeros((0, 38))
    assert apply_host(cfg, one, pts(), count_only=True) == (1, 0)
    # 1: no base list; times negative or not strictly increasing
    assert apply_host(cfg, empty, pts(), count_only=True) == (0, 1)
    assert apply_host(cfg, empty, pts(8.0), count_only=True) == (0, 1)
    two = event_lists.random_event_table(2, n_events=2)
    for t0, t1 in ((-4, 8), (8, 8), (8, 4)):
        bad = two.copy()
        bad[:, 0] = t0, t1
        assert apply_host(cfg, bad, pts(), count_only=True) == (0, 1)
    # 2: 65 points (64 are taken); the count is looked at before any point is
    wide = event_lists.random_event_table(3, n_events=2)
    wide[1, 0] = 400
    assert apply_host(cfg, wide, pts(*(4.0 * j for j in range(64))), count_only=True) == (64 + 1, 0)  # 0 and 400 are events
    assert apply_host(cfg, wide, pts(*(4.0 * j for j in range(65))), count_only=True) == (0, 2)
    assert apply_host(cfg, wide, pts(*([np.nan] * 65)), count_only=True) == (0, 2)
    # 3: behind duration + cp, or not finite; exactly duration + cp is taken
    assert apply_host(cfg, one, pts(104.0), count_only=True) == (2, 0)
    assert apply_host(cfg, one, pts(104.0 + 2.0 ** -40), count_only=True) == (0, 3)
    assert apply_host(cfg, one, pts(105.0), count_only=True) == (0, 3)
    for t in (np.nan, np.inf, -np.inf):
        assert apply_host(cfg, one, pts(t), count_only=True) == (0, 3)
    assert apply_host(cfg, one, pts(-1e300), count_only=True) == (1, 0)     # clamped to 0, where the event lies
    # ... also where the list ends within 100 ms of the largest int: no overflow, and a time no int holds is refused
    far = two.copy()
    far[:, 0] = 0, 2 ** 31 - 4
    assert apply_host(cfg, far, pts(float(2 ** 31 - 5)), count_only=True) == (3, 0)
    assert apply_host(cfg, far, pts(float(2 ** 31 - 1)), count_only=True) == (2, 0)   # rounded down to the period of the last event
    assert apply_host(cfg, far, pts(float(2 ** 31)), count_only=True) == (0, 3)
    assert apply_host(cfg, far, pts(float(2 ** 31) + 50.0), count_only=True) == (0, 3)
    # 4: two points in one control period, or going back; 3 is looked for in every point first
    assert apply_host(cfg, one, pts(8.0, 11.5), count_only=True) == (0, 4)
    assert apply_host(cfg, one, pts(8.0, 4.0), count_only=True) == (0, 4)
    assert apply_host(cfg, one, pts(8.0, 12.0), count_only=True) == (3, 0)
    assert apply_host(cfg, one, pts(8.0, 8.5, 200.0), count_only=True) == (0, 3)
    assert apply_host(product_config(cases.cfg(1)), one, pts(8.0, 9.0), count_only=True) == (3, 0)  # (at cp 1 they are apart)
    # a refused utterance writes nothing
    out = np.zeros(4, dtype=capi.EVENT_DTYPE)
    out["time_ms"] = 77
    assert raw_apply(cfg, capi.events_from_table(one), 1, capi.points_from_table(pts(8.0, 9.0)), 2, out, 4) == (0, 4)
    assert (out["time_ms"] == 77).all()


def test_bad_calls_return_minus_one():
    cfg = product_config(cases.cfg(4))
    ev = capi.events_from_table(event_lists.random_event_table(1, n_events=3))
    ev["time_ms"] = 0, 20, 40
    pt = capi.points_from_table([[10.0, 1.0, 0.0], [50.0, 2.0, 0.0]])                # new events at 8 and 48
    out = np.zeros(8, dtype=capi.EVENT_DTYPE)
    lib = g.load_library()
    assert raw_apply(cfg, ev, 3, pt, 2, out, 8) == (5, 0)
    assert raw_apply(None, ev, 3, pt, 2, out, 8)[0] == -1
    assert raw_apply(cfg, ev, 3, pt, 2, out, 8, status=False)[0] == -1
    assert raw_apply(cfg, None, 3, pt, 2, out, 8)[0] == -1
    assert raw_apply(cfg, ev, 3, None, 2, out, 8)[0] == -1
    assert raw_apply(cfg, ev, 3, pt, 2, out, 4)[0] == -1 and b"capacity" in lib.gvtm_last_error()
    assert raw_apply(cfg, ev, 3, None, 0, out, 3) == (3, 0)                  # no points: a null pointer is fine
    assert raw_apply(cfg, None, 0, None, 0, None, 0) == (0, 1)               # no events either: refused, not a bad call
    assert raw_apply(cfg, ev, 3, pt, 2, None, 0) == (5, 0)                   # count only: capacity is not read
    # a configuration gvtm_tracks_frame_count would refuse
    for field, value in (("control_period_ms", 0), ("reserved_", 1), ("drift_lowpass_cutoff", 1e6)):
        bad = product_config(cases.cfg(4))
        setattr(bad, field, value)
        assert raw_apply(bad, ev, 3, pt, 2, out, 8)[0] == -1
        assert lib.gvtm_tracks_frame_count(ctypes.byref(bad), capi._ptr(ev), 3) == ctypes.c_size_t(-1).value
    with pytest.raises(capi.GvtmError):
        capi.intonation_apply_host(cfg, ev, pt, capacity=4)


def test_restatement_agrees_with_the_host_entry_on_random_cases():
    statuses = {}
    for seed in range(300):
        table, points, cp, smooth = cases.random_case(seed)
        want, want_status = cases.apply_rule(table, points, cp, smooth)
        merged, status = apply_host(product_config(cases.cfg(cp, 1, 1, 1, smooth)), table, points)
        assert status == want_status, seed
        got = cases.events_to_table(merged)
        assert got.shape == want.shape and got.tobytes() == np.ascontiguousarray(want).tobytes(), seed
        statuses[status] = statuses.get(status, 0) + 1
    assert statuses.get(0, 0) >= 150 and statuses.get(3, 0) >= 10 and statuses.get(4, 0) >= 10, statuses


def test_names_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "gama_vtm.h")).read()
    symbols = subprocess.run(["nm", "-D", "--defined-only", capi.library_path()], check=True, capture_output=True, text=True).stdout
    for name in ENTRIES:
        assert re.search(r"\b%s\(" % name, header), name
        assert re.search(r" T %s$" % name, symbols, re.M), name
    assert "gvtm_intonation_point" in header and re.search(r"#define GVTM_MAX_INTONATION_POINTS 64\b", header)
    assert capi.POINT_DTYPE.itemsize == 24 and capi.MAX_INTONATION_POINTS == cases.MAX_POINTS == 64


def device_entries(plan, batch=2, null=None, n_lists=None, list_ids=True):
    """Status of the two device entries on a small (host-memory, never dereferenced) batch; null: an argument to leave out."""
    lib = plan._lib
    a = dict(events=np.zeros(4, dtype=capi.EVENT_DTYPE), list_offsets=np.array([0, 2, 4], dtype=np.int64), points=np.zeros(2, capi.POINT_DTYPE),
             point_offsets=np.array([0, 1, 2], dtype=np.int64), voice_ids=np.zeros(2, dtype=np.int32), events_out=np.zeros(6, dtype=capi.EVENT_DTYPE),
             offsets_out=np.zeros(3, dtype=np.int64), audio=np.zeros((2, 65536), dtype=np.float32))
    ids = np.zeros(2, dtype=np.int32) if list_ids else None
    p = {k: (None if k == null else v.ctypes.data) for k, v in a.items()}
    n_lists = 2 if n_lists is None else n_lists
    apply = lib.gvtm_apply_intonation_device(plan._h, p["events"], p["list_offsets"], n_lists, capi._ptr(ids), p["points"], p["point_offsets"],
                                             p["voice_ids"], batch, p["events_out"], 6, p["offsets_out"], None, None)
    synth = lib.gvtm_synthesize_intonation_device(plan._h, p["events"], p["list_offsets"], n_lists, capi._ptr(ids), p["points"], p["point_offsets"],
                                                  p["voice_ids"], 6, batch, 8, p["audio"], 65536, None, None, None, None, None, None)
    return apply, synth


def test_device_entries_check_their_arguments_and_then_want_a_device():
    plans = [g.VoicesPlan(configs(), 250.0, capi.DEVICE_NONE), male_plan(device=capi.DEVICE_NONE)]
    for plan, tracks in zip(plans, (track_configs(), track_configs(names=["male"]))):
        lib = plan._lib
        assert device_entries(plan) == (INVALID_ARGUMENT, INVALID_ARGUMENT)
        assert "gvtm_plan_set_voice_tracks" in lib.gvtm_last_error().decode()
        plan.set_voice_tracks(tracks)
        # every null is refused before the missing device is
        for null in ("events", "list_offsets", "points", "point_offsets", "voice_ids"):
            assert device_entries(plan, null=null) == (INVALID_ARGUMENT, INVALID_ARGUMENT), null
        assert device_entries(plan, null="events_out") == (INVALID_ARGUMENT, NO_DEVICE)  # (the one-call entry has its own)
        assert device_entries(plan, null="offsets_out") == (INVALID_ARGUMENT, NO_DEVICE)
        # without list ids every utterance has its own list
        assert device_entries(plan, list_ids=False) == (NO_DEVICE, NO_DEVICE)
        assert device_entries(plan, list_ids=False, n_lists=1) == (INVALID_ARGUMENT, INVALID_ARGUMENT)
        assert device_entries(plan, n_lists=1) == (NO_DEVICE, NO_DEVICE)             # with ids lists may be shared
        assert device_entries(plan) == (NO_DEVICE, NO_DEVICE)
        assert device_entries(plan, batch=0, null="events") == (NO_DEVICE, NO_DEVICE)  # as the neighbouring entries: no device, no call
    lib = g.load_library()
    assert lib.gvtm_apply_intonation_device(None, None, None, 0, None, None, None, None, 0, None, 0, None, None, None) == INVALID_ARGUMENT
    assert lib.gvtm_synthesize_intonation_device(None, None, None, 0, None, None, None, None, 0, 0, 0, None, 0, None, None, None, None, None, None) == INVALID_ARGUMENT
