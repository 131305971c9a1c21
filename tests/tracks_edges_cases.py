"""The event lists and generateOutput() settings of tests/golden/tracks_edges_golden.npz: lists built to reach the edges of
the device track kernel (gama_tts_amd/csrc/vtm_tracks.hip) -- lengths around its LDS table (kTableEvents = 240), columns
whose next set event lies far away, long lists, times off the control-period grid, several events inside one period,
control periods 1 to 4, intonation corner cases and every flag combination.  The fixture holds the reference's frames
for every call of every list and the SHA-256 of each list, so a generator that drifts is caught before the frames are."""
import hashlib

import numpy as np

import event_lists

# frames of a call up to this many are stored whole; longer calls as SHA-256 plus every FRAME_STRIDE-th frame
FULL_FRAMES = 600
FRAME_STRIDE = 16

# the 16 combinations of (macro, micro, drift, smooth)
FLAGS16 = [tuple((k >> b) & 1 for b in (3, 2, 1, 0)) for k in range(16)]


def cfg(cp=4, macro=1, micro=1, drift=1, smooth=1):
    """The 10 numbers of a call (oracle.track_config): the captured voice's pitches and drift settings, the drift generator
    at the control rate."""
    return np.array([cp, macro, micro, drift, smooth, -20.0, -16.0, 4.0, 1000.0 / cp, 4.0])


def _off_grid(t, cp):
    """Moves every time but the first off the control-period grid (a time on the grid gets 1 ms more), so that no boundary
    ever finds an event at exactly the current time: the deltas divide by times that are off the grid, never by 0."""
    t = t.copy()
    on = (t[1:, 0] % cp) == 0
    t[1:, 0][on] += 1
    assert (np.diff(t[:, 0]) >= 0).all()
    return t


def _far_gaps(n=1000):
    """~1,000 events; parameter 12 and special parameter 7 set at events with gaps of up to 380 between them."""
    rows_p = [0, 40, 420, 421, 700, n - 1]
    rows_s = [0, 10, 310, 311, 690, n - 1]
    return event_lists.random_event_table(1000, n_events=n, force_set={12: rows_p, 16 + 7: rows_s},
                                          force_unset={12: np.setdiff1d(np.arange(n), rows_p),
                                                       16 + 7: np.setdiff1d(np.arange(n), rows_s)})


def _unset_first():
    """Event 0 leaves parameter 3 unset (+inf), later events set it."""
    return event_lists.random_event_table(700, n_events=60, force_unset={3: [0]}, force_set={3: [5, 30]})


def _interp(last_only):
    t = event_lists.random_event_table(710 + last_only, n_events=80)
    t[:, 1] = 0.0
    if last_only:
        t[-1, 1] = 1.0
        t[-1, 2:6] = 2e-7, -3e-4, 0.02, 1.5
    return t


def _lists():
    L = {}
    for n in (239, 240, 241, 242):
        L["b%d" % n] = (lambda g, n=n: event_lists.boundary_table(n, seed=n),
                        [cfg(), cfg(4, 0, 1, 1, 0), cfg(4, 1, 0, 0, 1)])
    L["joined2600"] = (lambda g: event_lists.joined_captured(g, 2600), [cfg(), cfg(4, 1, 1, 1, 0)])
    L["far1000"] = (lambda g: _far_gaps(), [cfg(), cfg(4, 0, 1, 1, 1)])
    for cp in (1, 2, 3, 4):
        # gaps of 1 ms up to two periods, off the grid: several events inside one period, deltas over negative times
        L["offgrid_cp%d" % cp] = (lambda g, cp=cp: _off_grid(event_lists.random_event_table(500 + cp, n_events=150, control_period=cp,
                                                                                             max_gap_periods=6, min_gap_ms=1), cp),
                                  [cfg(cp), cfg(cp, 1, 1, 1, 0)])
        # gaps from 0: events that share a time, and boundaries that find an event at exactly the current time (0 / 0, x / 0)
        L["subperiod_cp%d" % cp] = (lambda g, cp=cp: event_lists.random_event_table(600 + cp, n_events=120, control_period=cp,
                                                                                    max_gap_periods=2, min_gap_ms=0),
                                    [cfg(cp), cfg(cp, 0, 1, 0, 1)])
    L["unset_first"] = (lambda g: _unset_first(), [cfg(), cfg(4, 1, 1, 0, 0)])
    L["interp_none"] = (lambda g: _interp(False), [cfg(), cfg(4, 1, 1, 1, 0)])
    L["interp_last"] = (lambda g: _interp(True), [cfg(), cfg(4, 1, 1, 1, 0)])
    L["flags16"] = (lambda g: event_lists.random_event_table(720, n_events=60), [cfg(4, *f) for f in FLAGS16])
    return L


LISTS = _lists()


def table(name, golden_tracks):
    return LISTS[name][0](golden_tracks)


def calls(name):
    return LISTS[name][1]


def table_sha256(t):
    return hashlib.sha256(np.ascontiguousarray(t, dtype="<f8").tobytes()).hexdigest()


def frames_sha256(frames):
    return hashlib.sha256(np.ascontiguousarray(frames, dtype="<f4").tobytes()).hexdigest()


def check_frames(fixture, name, call, frames):
    """frames (float32 [F][16]) against call `call` of list `name` of the fixture, bit for bit: whole, or SHA-256 plus
    strided frames.  Returns None if they match, else a message."""
    key = "%s__%d" % (name, call)
    n = int(fixture[key + "__count"])
    if frames.shape != (n, 16):
        return "%s: %s frames, fixture %d" % (key, frames.shape, n)
    if key + "__frames" in fixture:
        want = fixture[key + "__frames"]
        if not np.array_equal(frames.view(np.uint32), want.view(np.uint32)):
            bad = np.argwhere(frames.view(np.uint32) != want.view(np.uint32))
            return "%s: %d values differ, first at %s" % (key, bad.shape[0], bad[0].tolist())
        return None
    want = fixture[key + "__strided"]
    if not np.array_equal(frames[::FRAME_STRIDE].view(np.uint32), want.view(np.uint32)):
        return "%s: strided frames differ" % key
    if frames_sha256(frames) != bytes(fixture[key + "__sha256"]).decode():
        return "%s: SHA-256 differs" % key
    return None
