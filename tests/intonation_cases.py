"""The cases of tests/golden/intonation_golden.npz -- base event lists, intonation points and settings run through the
reference's clearMacroIntonation(), prepareMacroIntonationInterpolation() and generateOutput()
(tests/golden/ref_intonation_table.cpp) -- and a restatement of the rule in Python floats (IEEE doubles, one rounding per
operation: no contraction to worry about) for fresh random cases.

Base lists: the captured "Hello world" lists with the cubic and with the linear contour of the text parser, made lists of 1
and 2 events, of 239, 240 and 241 events (the merged lists straddle the tracks kernel's LDS table of 240), of 300 events,
lists with times off the control-period grid at control periods 1 to 4, and a list whose first event is not at time 0 with a
point in front of it.  Points: none, 1, 2, 12 and 64 of them, on event times, between events, after the last event up to
exactly duration + cp (the last time insertEvent accepts), and at a negative time (absoluteTime() clamps it to 0)."""
import hashlib
import math
import zlib

import numpy as np

import event_lists
import tracks_edges_cases

MAX_POINTS = 64  # GVTM_MAX_INTONATION_POINTS
# frames of a case up to this many are stored whole; longer cases as SHA-256 plus every FRAME_STRIDE-th frame
FULL_FRAMES = 400
FRAME_STRIDE = 16

cfg = tracks_edges_cases.cfg


# ---- the rule, restated ----

def point_time(time_ms, cp, last_time):
    """-> q, or None where insertEvent returns null (EventList.cpp:302-315)."""
    if not math.isfinite(time_ms):
        return None
    t = 0.0 if time_ms < 0.0 else time_ms
    if t > float(last_time + 100 + cp) or t >= 2.0 ** 31:  # (no int holds the time: refused like one behind the list)
        return None
    q = int(t)
    if cp != 1:
        q -= q % cp
    return q


# the cubic's four coefficients (a, b, c, d) as signed products of the segment's numbers, in the order the reference adds them
# (EventList.cpp:863-870): (sign, factors multiplied from the left); p1, c1 / p2, c2 are x1's / x2's square and cube
_CUBIC = (
    ((-1, (2.0, "y2")), (-1, ("m1", "x1")), (-1, ("m2", "x1")), (+1, (2.0, "y1")), (+1, ("m1", "x2")), (+1, ("m2", "x2"))),
    ((+1, (3.0, "y2", "x1")), (+1, ("m1", "p1")), (+1, (2.0, "m2", "p1")), (-1, (3.0, "x1", "y1")), (+1, (3.0, "x2", "y2")),
     (+1, ("m1", "x1", "x2")), (-1, ("m2", "x1", "x2")), (-1, (3.0, "y1", "x2")), (-1, (2.0, "m1", "p2")), (-1, ("m2", "p2"))),
    ((-1, ("m2", "c1")), (-1, (6.0, "y2", "x1", "x2")), (-1, (2.0, "m1", "p1", "x2")), (-1, ("m2", "p1", "x2")),
     (+1, (6.0, "x1", "y1", "x2")), (+1, ("m1", "x1", "p2")), (+1, (2.0, "m2", "x1", "p2")), (+1, ("m1", "c2"))),
    ((-1, ("y2", "c1")), (+1, (3.0, "y2", "p1", "x2")), (+1, ("m2", "c1", "x2")), (+1, ("m1", "p1", "p2")), (-1, ("m2", "p1", "p2")),
     (-1, (3.0, "x1", "y1", "p2")), (-1, ("m1", "x1", "c2")), (+1, ("y1", "c2"))),
)


def segment(smooth, x1, y1, m1, x2, y2, m2):
    """The polynomial of the segment (x1, y1, m1) -> (x2, y2, m2) in Python floats, one rounding per operation: every
    product from the left, every sum from the left, then times 1 / dx^3 (negating a product is exact, so a leading minus
    is the same as the reference's negative literal or negated product)."""
    v = dict(x1=float(x1), y1=float(y1), m1=float(m1), x2=float(x2), y2=float(y2), m2=float(m2))
    dx = v["x2"] - v["x1"]
    if not smooth:
        rise = (v["y2"] - v["y1"]) / dx
        return rise, v["y1"] - v["x1"] * rise, 0.0, 0.0
    v["p1"] = v["x1"] * v["x1"]
    v["c1"] = v["p1"] * v["x1"]
    v["p2"] = v["x2"] * v["x2"]
    v["c2"] = v["p2"] * v["x2"]
    scale = 1.0 / (dx * dx * dx)
    out = []
    for terms in _CUBIC:
        total = None
        for sign, factors in terms:
            product = None
            for f in factors:
                f = v[f] if isinstance(f, str) else f
                product = f if product is None else product * f
            if total is None:
                total = -product if sign < 0 else product
            else:
                total = total - product if sign < 0 else total + product
        out.append(total * scale)
    return tuple(out)


def apply_rule(table, points, cp, smooth):
    """table float64 [E][38], points float64 [P][3] -> (merged table float64 [M][38], status); a refused utterance has
    M = 0.  The statuses and their order are gvtm_intonation_apply_host's."""
    table = np.asarray(table, dtype=np.float64).reshape(-1, 38)
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    none = np.zeros((0, 38))
    times = table[:, 0].astype(np.int64)
    if table.shape[0] == 0 or times[0] < 0 or (np.diff(times) <= 0).any():
        return none, 1
    if points.shape[0] > MAX_POINTS:
        return none, 2
    q = [point_time(float(p[0]), cp, int(times[-1])) for p in points]
    if any(v is None for v in q):
        return none, 3
    if any(q[j] <= q[j - 1] for j in range(1, len(q))):
        return none, 4
    rows = {int(t): row.copy() for t, row in zip(times, table)}
    for v in q:
        if v not in rows:
            rows[v] = np.concatenate([[float(v)], np.zeros(5), np.full(32, np.inf)])
    for row in rows.values():
        row[1:6] = 0.0
    if len(q) >= 2:
        for j, v in enumerate(q):
            rows[v][1] = 1.0
            if j + 1 < len(q):
                rows[v][2:6] = segment(smooth, v, points[j, 1], points[j, 2], q[j + 1], points[j + 1, 1], points[j + 1, 2])
            else:
                rows[v][2:6] = (0.0, 0.0, 0.0, points[j, 1]) if smooth else (0.0, points[j, 1], 0.0, 0.0)
    return np.array([rows[t] for t in sorted(rows)]), 0


# ---- points ----

def make_points(table, cp, n, mode, seed):
    """n points for the base list `table`, their events on distinct control periods in increasing order.
      on       on the times of base events (rounded down to the grid where those are off it)
      between  on periods no base event lies in, the times off the grid (fractions of a millisecond included)
      mix      anywhere up to duration + cp
      after    half of them behind the last event, the last at exactly duration + cp
      neg      mix, the first at a negative time
      front    mix, the first in front of the first base event (which must not lie in the first period)"""
    if n == 0:
        return np.zeros((0, 3))
    rng = np.random.default_rng([seed, n, cp])
    times = table[:, 0].astype(np.int64)
    last_slot = int(times[-1] + 100 + cp) // cp
    base_slots = np.unique(times // cp)
    if mode == "on":
        slots = rng.choice(base_slots, n, replace=False)
    elif mode == "between":
        slots = rng.choice(np.setdiff1d(np.arange(last_slot), base_slots), n, replace=False)
    elif mode == "after":
        front, behind = np.arange(int(times[-1]) // cp + 1), np.arange(int(times[-1]) // cp + 1, last_slot)
        n_front = max(min((n - 1) - (n - 1) // 2, front.size), n - 1 - behind.size)
        slots = np.concatenate([rng.choice(front, n_front, replace=False), rng.choice(behind, n - 1 - n_front, replace=False), [last_slot]])
    else:
        slots = rng.choice(np.arange(1, last_slot), n, replace=False)
    slots = np.sort(slots)
    if mode == "front":
        assert times[0] >= cp
        slots[0] = 0
    assert np.unique(slots).size == n
    p = np.zeros((n, 3))
    p[:, 0] = slots * cp
    if mode != "on":
        p[:, 0] += rng.uniform(0.0, cp, n) * (rng.random(n) < 0.8)  # most off the grid, some on it
        p[:, 0] = np.minimum(p[:, 0], slots * cp + cp - 2.0 ** -20)
    if mode == "after":
        p[-1, 0] = float(times[-1] + 100 + cp)
    if mode == "neg":
        slots[0] = 0
        p[0, 0] = -37.5
    p[:, 1] = rng.uniform(-12.0, 6.0, n)
    p[:, 2] = rng.uniform(-0.08, 0.08, n)
    return p


# ---- base lists and cases ----

def _offgrid(cp):
    """Times off the control-period grid, gaps from 1 ms (several events inside one period), strictly increasing."""
    t = tracks_edges_cases._off_grid(event_lists.random_event_table(930 + cp, n_events=40, control_period=cp, max_gap_periods=6, min_gap_ms=1), cp)
    for i in range(1, t.shape[0]):
        t[i, 0] = max(t[i, 0], t[i - 1, 0] + 1)
    return t


def _late():
    t = event_lists.random_event_table(901, n_events=30)
    t[:, 0] += 40
    return t


BASES = {
    "hello0": lambda g: g["hello__0__events"].copy(),   # captured under the cubic contour
    "hello5": lambda g: g["hello__5__events"].copy(),   # ... and under the linear one
    "one": lambda g: event_lists.random_event_table(910, n_events=1),
    "two": lambda g: event_lists.random_event_table(911, n_events=2),
    "b239": lambda g: event_lists.boundary_table(239, seed=239),
    "b240": lambda g: event_lists.boundary_table(240, seed=240),
    "b241": lambda g: event_lists.boundary_table(241, seed=241),
    "r300": lambda g: event_lists.random_event_table(900, n_events=300),
    "late": lambda g: _late(),
    "off1": lambda g: _offgrid(1),
    "off2": lambda g: _offgrid(2),
    "off3": lambda g: _offgrid(3),
    "off4": lambda g: _offgrid(4),
}

# name: (base list, control period, smooth, points, mode)
CASES = {
    "hello0_p0": ("hello0", 4, 1, 0, "mix"),
    "hello0_p1": ("hello0", 4, 1, 1, "between"),
    "hello0_p2_on": ("hello0", 4, 1, 2, "on"),
    "hello0_p12": ("hello0", 4, 1, 12, "mix"),
    "hello0_p12_on": ("hello0", 4, 1, 12, "on"),
    "hello0_p12_between": ("hello0", 4, 1, 12, "between"),
    "hello0_p12_lin": ("hello0", 4, 0, 12, "mix"),
    "hello0_p12_after": ("hello0", 4, 1, 12, "after"),
    "hello0_p12_neg": ("hello0", 4, 0, 12, "neg"),
    "hello0_p64": ("hello0", 4, 1, 64, "mix"),
    "hello5_p2": ("hello5", 4, 0, 2, "between"),
    "hello5_p12": ("hello5", 4, 0, 12, "mix"),
    "hello5_p12_smooth": ("hello5", 4, 1, 12, "after"),
    "one_p0": ("one", 4, 1, 0, "mix"),
    "one_p1": ("one", 4, 1, 1, "between"),
    "one_p2_after": ("one", 4, 1, 2, "after"),
    "one_p12_lin": ("one", 2, 0, 12, "after"),
    "two_p1": ("two", 4, 1, 1, "between"),
    "two_p2_on": ("two", 4, 0, 2, "on"),
    "two_p12": ("two", 4, 1, 12, "mix"),
    "b239_p1": ("b239", 4, 1, 1, "between"),
    "b239_p2": ("b239", 4, 0, 2, "between"),
    "b240_p0": ("b240", 4, 1, 0, "mix"),
    "b240_p1": ("b240", 4, 1, 1, "between"),
    "b241_p2_on": ("b241", 4, 1, 2, "on"),
    "b241_p12": ("b241", 4, 0, 12, "mix"),
    "r300_p64": ("r300", 4, 1, 64, "mix"),
    "r300_p64_lin": ("r300", 4, 0, 64, "between"),
    "late_p1_front": ("late", 4, 1, 1, "front"),
    "late_p12_front": ("late", 4, 1, 12, "front"),
    "late_p2_neg": ("late", 4, 0, 2, "neg"),
    "off1_p12": ("off1", 1, 1, 12, "mix"),
    "off1_p12_lin": ("off1", 1, 0, 12, "after"),
    "off2_p12": ("off2", 2, 1, 12, "mix"),
    "off2_p64": ("off2", 2, 1, 64, "mix"),
    "off3_p12": ("off3", 3, 1, 12, "mix"),
    "off3_p12_lin": ("off3", 3, 0, 12, "neg"),
    "off4_p12": ("off4", 4, 1, 12, "on"),
    "off4_p2_after": ("off4", 4, 0, 2, "after"),
}


def bases(golden_tracks):
    return {n: make(golden_tracks) for n, make in BASES.items()}


def case(name, base_tables):
    """-> (base table, points [P][3], the 10 numbers of the call)"""
    base, cp, smooth, n, mode = CASES[name]
    table = base_tables[base]
    return table, make_points(table, cp, n, mode, zlib.crc32(name.encode())), cfg(cp, 1, 1, 1, smooth)


def random_case(seed):
    """A fresh case for the restatement against the host entry: (table, points, cp, smooth).  About one in four breaks
    a rule (statuses 3 and 4); the rest are valid."""
    rng = np.random.default_rng([seed, 77])
    cp = int(rng.integers(1, 5))
    smooth = int(rng.integers(0, 2))
    table = event_lists.random_event_table(20000 + seed, n_events=int(rng.integers(1, 40)), control_period=cp, max_gap_periods=6,
                                           min_gap_ms=1 if seed % 2 else None)
    table[:, 0] += int(rng.integers(0, 3)) * 7
    last_slot = int(table[-1, 0] + 100 + cp) // cp
    n = int(rng.integers(0, min(MAX_POINTS, last_slot - 1) + 1))
    p = make_points(table, cp, n, "mix", 30000 + seed)
    kind = rng.integers(0, 8)
    if n >= 2 and kind == 0:
        p[n // 2, 0] = p[n // 2 - 1, 0]          # two points in one control period
    elif n >= 1 and kind == 1:
        p[-1, 0] = table[-1, 0] + 100 + cp + 0.5  # behind the last time insertEvent accepts
    return table, p, cp, smooth


# ---- the fixture ----

def sha256(a, dtype):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=dtype).tobytes()).hexdigest()


def events_to_table(events):
    """gvtm_event records (capi.EVENT_DTYPE) -> float64 [M][38]"""
    t = np.zeros((events.shape[0], 38))
    t[:, 0] = events["time_ms"]
    t[:, 1] = events["has_interp"]
    t[:, 2:6] = events["interp"]
    t[:, 6:22] = events["param"]
    t[:, 22:38] = events["special"]
    return t


def check_merged(fixture, name, merged):
    """merged float64 [M][38] against the reference's list of case `name`, bit for bit: times, has_interp, the four doubles
    and the SHA-256 of the whole table.  Returns None if they match, else a message."""
    want_time = fixture[name + "__time"]
    if merged.shape[0] != want_time.shape[0]:
        return "%s: %d merged events, fixture %d" % (name, merged.shape[0], want_time.shape[0])
    if not np.array_equal(merged[:, 0], want_time.astype(np.float64)):
        return "%s: times differ" % name
    if not np.array_equal(merged[:, 1], fixture[name + "__has_interp"].astype(np.float64)):
        return "%s: has_interp differs" % name
    got, want = np.ascontiguousarray(merged[:, 2:6]).view(np.int64), fixture[name + "__interp"].view(np.int64)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        return "%s: %d polynomial coefficients differ, first at %s" % (name, bad.shape[0], bad[0].tolist())
    if sha256(merged, "<f8") != bytes(fixture[name + "__sha256"]).decode():
        return "%s: SHA-256 of the merged table differs" % name
    return None


def check_frames(fixture, name, frames):
    """frames float32 [F][16] against the reference's for case `name`, bit for bit -- except that where the reference's
    frame is NaN the frame must be NaN, of any sign and payload: inf - inf and 0 / 0 give the x86 default NaN (sign bit set)
    in the reference's build and the device's default NaN on the device (the rule of tests/test_gpu_tracks_edges.py; a list
    with a point in front of its first event starts from an event that sets nothing, so its values are +infinity and then
    NaN).  Cases stored as SHA-256 plus strided frames compare the hash only where no frame is NaN.  Returns None if they
    match, else a message."""
    n = int(fixture[name + "__count"])
    if frames.shape != (n, 16):
        return "%s: %s frames, fixture %d" % (name, frames.shape, n)
    whole = name + "__frames" in fixture
    want = fixture[name + "__frames"] if whole else fixture[name + "__strided"]
    got = frames if whole else frames[::FRAME_STRIDE]
    wn = np.isnan(want)
    if not np.array_equal(np.isnan(got), wn):
        return "%s: NaN in other places than the reference's" % name
    diff = (got.view(np.uint32) != want.view(np.uint32)) & ~wn
    if diff.any():
        bad = np.argwhere(diff)
        return "%s: %d values differ, first at %s" % (name, bad.shape[0], bad[0].tolist())
    if not whole and not np.isnan(frames).any() and sha256(frames, "<f4") != bytes(fixture[name + "__frames_sha256"]).decode():
        return "%s: SHA-256 of the frames differs" % name
    return None
