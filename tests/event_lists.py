"""Event lists for the track-generation tests: the captured fixtures and a synthetic generator."""
import numpy as np


def load_golden(golden_tracks, name, call):
    cfg = golden_tracks["%s__%d__cfg" % (name, call)]
    return cfg, golden_tracks["%s__%d__events" % (name, call)], golden_tracks["%s__%d__frames" % (name, call)]


def random_event_table(seed, n_events=40, control_period=4, max_gap_periods=12, min_gap_ms=None, special_rate=0.08,
                       force_set=None, force_unset=None):
    """A synthetic event list in the 38-column form: increasing times (multiples of the control period), every
    parameter set on the first event, later events setting a random subset (+inf = not set), occasional special
    parameters, macro-intonation polynomials on some events.

    The defaults draw exactly what they always drew.  Edges on request:
      min_gap_ms   gaps drawn in whole milliseconds from [min_gap_ms, max_gap_periods * control_period] instead of whole
                   control periods: times off the control-period grid, and (min_gap_ms < control_period) several events
                   inside one period; 0 lets events share a time
      special_rate chance that an event sets a special parameter: one number, or 16 of them (one per special column,
                   0: never set)
      force_set / force_unset  {column: event indices}, column 0..15 parameters, 16..31 special parameters: these events
                   set (with a value of their own) / leave unset the column, whatever was drawn"""
    rng = np.random.default_rng(seed)
    t = np.zeros((n_events, 38))
    time = 0
    for i in range(n_events):
        if i:
            if min_gap_ms is None:
                time += control_period * int(rng.integers(1, max_gap_periods + 1))
            else:
                time += int(rng.integers(min_gap_ms, max_gap_periods * control_period + 1))
        t[i, 0] = time
        t[i, 6:38] = np.inf
        has = rng.random(16) < (1.0 if i == 0 else 0.55)
        vals = np.concatenate([rng.uniform(-10, 2, 1), rng.uniform(0, 60, 3), rng.uniform(0, 7, 1), rng.uniform(100, 5500, 1),
                               rng.uniform(250, 4500, 1), rng.uniform(0.1, 3.0, 8), rng.uniform(0.1, 1.5, 1)])
        t[i, 6:22][has] = vals[has]
        sp = rng.random(16) < (0.08 if special_rate is None else np.asarray(special_rate))
        t[i, 22:38][sp] = rng.uniform(-2, 2, 16)[sp]
        if rng.random() < 0.3:
            t[i, 1] = 1.0
            t[i, 2:6] = rng.uniform(-1e-6, 1e-6), rng.uniform(-1e-3, 1e-3), rng.uniform(-0.05, 0.05), rng.uniform(-6, 6)
    if force_set or force_unset:
        extra = np.random.default_rng([seed, 38])  # the table above stays what the defaults make
        for c, rows in (force_set or {}).items():
            rows = np.asarray(rows, dtype=np.int64)
            lo, hi = (-2.0, 2.0) if c >= 16 else _PARAM_RANGE[c]
            t[rows, 6 + c] = extra.uniform(lo, hi, rows.size)
        for c, rows in (force_unset or {}).items():
            t[np.asarray(rows, dtype=np.int64), 6 + c] = np.inf
    return t


# the ranges random_event_table draws parameter values from
_PARAM_RANGE = [(-10, 2), (0, 60), (0, 60), (0, 60), (0, 7), (100, 5500), (250, 4500)] + [(0.1, 3.0)] * 8 + [(0.1, 1.5)]

# boundary_table's column layouts (columns as in force_set: 0..15 parameters, 16..31 special parameters)
FAR_PARAM = 9            # set on the first two events and on the last one only
NEVER_SPECIAL = 16 + 3   # never set
FIRST_SPECIAL = 16 + 5   # set on the first event only
FAR_SPECIAL = 16 + 11    # set on the first and on the last event only


def boundary_table(n, seed=0, control_period=4, min_gap_ms=None):
    """An event list of n events whose columns reach as far as a list of n events allows: special parameter FAR_SPECIAL set
    on events 0 and n - 1 only, parameter FAR_PARAM on events 0, 1 and n - 1 only (every parameter is set on event 0, and
    the search for the next set event starts at the boundary after the event that set it: these two searches run n - 2
    events), special parameter NEVER_SPECIAL never set, FIRST_SPECIAL on event 0 only; the other columns as
    random_event_table draws them (special parameters at rate 0.3, so that every other special column changes often)."""
    if n < 3:
        return random_event_table(seed, n_events=n, control_period=control_period, min_gap_ms=min_gap_ms)
    rate = np.full(16, 0.3)
    for c in (NEVER_SPECIAL, FIRST_SPECIAL, FAR_SPECIAL):
        rate[c - 16] = 0.0
    ends = sorted({0, n - 1})
    return random_event_table(seed, n_events=n, control_period=control_period, min_gap_ms=min_gap_ms, special_rate=rate,
                              force_set={FAR_PARAM: sorted({0, 1, n - 1}), FAR_SPECIAL: ends, FIRST_SPECIAL: [0]},
                              force_unset={FAR_PARAM: np.arange(2, n - 1)})


CAPTURED = ("hello", "fox", "question", "count")


def joined_captured(golden_tracks, n_events, gap_ms=60):
    """A realistic long event list: the reference's own captured lists (call 0 of tracks_golden.npz: text parser, rules,
    intonation) back to back, each shifted to start gap_ms after the one before ends, cut at n_events."""
    parts, start, k = [], 0, 0
    while sum(p.shape[0] for p in parts) < n_events:
        e = golden_tracks["%s__0__events" % CAPTURED[k % len(CAPTURED)]].copy()
        e[:, 0] += start
        start = int(e[-1, 0]) + gap_ms
        parts.append(e)
        k += 1
    return np.concatenate(parts)[:n_events].copy()
