"""Intonation contours applied to event lists on the device (gvtm_apply_intonation_device, vtm_intonation.hip): merged lists,
offsets and statuses bit for bit gvtm_intonation_apply_host's on every case of tests/golden/intonation_golden.npz, in
batches of 1, 2, 3 and 67, with lists of their own and with one base list shared, under voices that differ in
smooth_intonation, with refused utterances of every status between good ones; the tracks kernel's frames on the
device-merged lists against the reference's generateOutput() after its own prepare; and the one-call entry
(gvtm_synthesize_intonation_device) against the calls made separately.

Everything is compared as bytes.  The output buffers start out as a guard pattern, and the whole buffer -- the lists'
room, the refused utterances' none, GUARD_EVENTS events behind out_capacity -- is compared with the pattern laid out on the
host, so anything written where nothing should be shows.  The frames follow the NaN rule of intonation_cases.check_frames."""
import os

import numpy as np
import pytest

import gama_tts_amd as g
from gama_tts_amd import capi
import intonation_cases as cases
from device_io import current_stream, filled, to_device, to_host
from track_cases import product_config, used_drift
from voice_cases import configs, configs5

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GUARD = 0xA5          # every byte of an output buffer before the call
GUARD_EVENTS = 8      # events behind out_capacity
SMOOTH, LINEAR = 0, 1  # voice ids of the two-voice plans below


@pytest.fixture(scope="module")
def fixture():
    z = np.load(os.path.join(HERE, "golden", "intonation_golden.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def base_tables(golden_tracks):
    return cases.bases(golden_tracks)


def track_pair(cp):
    """Two configurations that differ in smooth_intonation alone: voice SMOOTH and voice LINEAR."""
    return [product_config(cases.cfg(cp, 1, 1, 1, 1)), product_config(cases.cfg(cp, 1, 1, 1, 0))]


@pytest.fixture(scope="module")
def plans():
    """cp -> a plan of two (male) voices at control period cp whose track configurations are track_pair(cp)."""
    made = {}

    def get(cp):
        if cp not in made:
            made[cp] = g.VoicesPlan(configs(names=["male", "male"]), 1000.0 / cp, 0)
            made[cp].set_voice_tracks(track_pair(cp))
        return made[cp]
    return get


class Batch:
    """Base lists (tables), per utterance its list, points [P][3] and voice; on the device as the entries take them."""

    def __init__(self, lists, points, voices, list_ids=None):
        self.lists, self.points, self.voices, self.list_ids = lists, points, np.asarray(voices, dtype=np.int32), list_ids
        self.batch = len(points)
        ev = [capi.events_from_table(t) for t in lists]
        self.list_offsets = np.zeros(len(lists) + 1, dtype=np.int64)
        self.list_offsets[1:] = np.cumsum([len(e) for e in ev])
        self.point_offsets = np.zeros(self.batch + 1, dtype=np.int64)
        self.point_offsets[1:] = np.cumsum([len(p) for p in points])
        pts = np.concatenate([np.asarray(p, dtype=np.float64).reshape(-1, 3) for p in points] + [np.zeros((1, 3))])  # (never empty)
        self.d_events, self.d_list_offsets, self.d_points, self.d_point_offsets, self.d_voices = to_device(
            np.concatenate(ev + [np.zeros(1, capi.EVENT_DTYPE)]).view(np.uint8), self.list_offsets, pts, self.point_offsets, self.voices)
        self.d_list_ids = None if list_ids is None else to_device(np.asarray(list_ids, dtype=np.int32))[0]

    def list_of(self, b):
        return b if self.list_ids is None else int(self.list_ids[b])

    def room(self):
        """What the header tells the caller to size the output with: the sum over b of E(list of b) + P_b."""
        return sum(self.lists[self.list_of(b)].shape[0] + len(self.points[b]) for b in range(self.batch) if 0 <= self.list_of(b) < len(self.lists))

    def expected(self, cp, capacity, n_voices=2):
        """The host entry utterance by utterance, laid out as the device lays the lists out -> (the output buffer's bytes,
        guard included; offsets; statuses; the merged record arrays)."""
        size = capi.EVENT_DTYPE.itemsize
        buf = np.full((capacity + GUARD_EVENTS) * size, GUARD, dtype=np.uint8)
        offsets, statuses, merged_all = np.zeros(self.batch + 1, dtype=np.int64), np.zeros(self.batch, dtype=np.int32), []
        at = 0
        for b in range(self.batch):
            l, v = self.list_of(b), int(self.voices[b])
            merged, status = np.zeros(0, capi.EVENT_DTYPE), 1
            if 0 <= l < len(self.lists) and 0 <= v < n_voices:
                pts = capi.points_from_table(self.points[b])
                if len(pts) > cases.MAX_POINTS:
                    status = 2 if self.lists[l].shape[0] else 1  # (the binding sizes its output from the counts: not called)
                else:
                    merged, status = capi.intonation_apply_host(track_pair(cp)[v], capi.events_from_table(self.lists[l]), pts)
            if status == 0 and at + len(merged) > capacity:
                merged, status = merged[:0], 5
            buf[at * size: (at + len(merged)) * size] = merged.view(np.uint8)
            at += len(merged)
            offsets[b + 1], statuses[b] = at, status
            merged_all.append(merged)
        return buf, offsets, statuses, merged_all

    def apply(self, plan, capacity, status=True):
        """gvtm_apply_intonation_device into guarded buffers -> (events out as bytes, guard included; offsets; statuses),
        still on the device."""
        size = capi.EVENT_DTYPE.itemsize
        d_out = filled((capacity + GUARD_EVENTS) * size, GUARD, np.uint8)
        d_offsets, d_status = filled(self.batch + 1, -7, np.int64), filled(self.batch, -9, np.int32)
        plan.apply_intonation_device(self.d_events, self.d_list_offsets, len(self.lists), self.d_list_ids, self.d_points, self.d_point_offsets,
                                     self.d_voices, self.batch, d_out, capacity, d_offsets, d_status if status else None, current_stream())
        return d_out, d_offsets, d_status


def check_apply(plan, cp, batch, capacity=None, what=""):
    capacity = batch.room() if capacity is None else capacity
    want_buf, want_off, want_status, merged = batch.expected(cp, capacity)
    got_buf, got_off, got_status = to_host(*batch.apply(plan, capacity))
    assert np.array_equal(got_status, want_status), (what, got_status.tolist(), want_status.tolist())
    assert np.array_equal(got_off, want_off), (what, got_off.tolist(), want_off.tolist())
    if not np.array_equal(got_buf, want_buf):
        bad = np.flatnonzero(got_buf != want_buf)
        event, byte = divmod(int(bad[0]), capi.EVENT_DTYPE.itemsize)
        raise AssertionError("%s: %d bytes differ, first in event %d of the output (capacity %d) at byte %d" % (what, bad.size, event, capacity, byte))
    return merged, want_status


def fixture_batch(names, base_tables):
    """The fixture's cases `names` as a batch, each with a list of its own; the voice by the case's smooth flag."""
    inputs = [cases.case(n, base_tables) for n in names]
    return Batch([t for t, _, _ in inputs], [p for _, p, _ in inputs], [SMOOTH if int(c[4]) else LINEAR for _, _, c in inputs])


def names_of(cp):
    return [n for n, c in cases.CASES.items() if c[1] == cp]


@pytest.mark.parametrize("cp", [1, 2, 3, 4])
def test_every_fixture_case_lists_and_frames(fixture, base_tables, plans, cp):
    """All cases of one control period in one batch: the device's lists are the host entry's and the reference's, and the
    tracks kernel's frames on them are the reference's generateOutput() after its own prepare."""
    names, plan = names_of(cp), plans(cp)
    batch = fixture_batch(names, base_tables)
    merged, _ = check_apply(plan, cp, batch, what="cp %d" % cp)
    for n, m in zip(names, merged):
        assert cases.check_merged(fixture, n, cases.events_to_table(m)) is None
    # frames: the merged lists and their offsets stay where the apply entry left them
    d_out, d_offsets, _ = batch.apply(plan, batch.room(), status=False)
    max_frames = max(int(fixture[n + "__count"]) for n in names)
    d_params, d_counts = filled((len(names), max_frames, 16), 7.0, np.float32), filled(len(names), 99, np.int32)
    plan.generate_tracks_voices_device(d_out, d_offsets, batch.d_voices, len(names), max_frames, d_params, d_counts, None, current_stream())
    params, counts = to_host(d_params, d_counts)
    for b, n in enumerate(names):
        assert counts[b] == int(fixture[n + "__count"]), n
        assert cases.check_frames(fixture, n, params[b, : counts[b]]) is None
        assert (params[b, counts[b]:] == 7.0).all(), n


@pytest.mark.parametrize("size", [1, 2, 3, 67])
def test_batches_of_own_lists(base_tables, plans, size):
    names = names_of(4)
    batch = fixture_batch([names[(5 * size + b) % len(names)] for b in range(size)], base_tables)
    check_apply(plans(4), 4, batch, what="batch %d" % size)


def contours(table, cp, count, seed):
    """`count` point sets for one base list: every point count of the fixture and every placement, in turn."""
    sizes, modes = (12, 0, 1, 2, 64, 5, 33), ("mix", "between", "on", "after", "neg")
    n_on = np.unique(table[:, 0].astype(np.int64) // cp).size  # ("on" has that many periods to choose from)
    return [cases.make_points(table, cp, sizes[i % len(sizes)], "mix" if modes[i % len(modes)] == "on" and sizes[i % len(sizes)] > n_on else modes[i % len(modes)],
                              seed + i) for i in range(count)]


def test_one_shared_list_under_67_contours_and_mixed_voices(base_tables, plans):
    table = base_tables["hello0"]
    points = contours(table, 4, 67, 100)
    voices = [(b // 3) % 2 for b in range(67)]
    shared = Batch([table], points, voices, list_ids=[0] * 67)
    merged, _ = check_apply(plans(4), 4, shared, what="shared")
    # the same utterances with a copy of the list each: the same bytes
    own = Batch([table] * 67, points, voices)
    again, _ = check_apply(plans(4), 4, own, what="own copies")
    assert all(a.tobytes() == m.tobytes() for a, m in zip(again, merged))
    # several lists shared unevenly, ids in no order
    lists = [base_tables[n] for n in ("hello0", "two", "b240", "late")]
    ids = [(7 * b) % 4 for b in range(67)]
    some = Batch(lists, [cases.make_points(lists[l], 4, (1, 2, 12)[b % 3], "mix", 200 + b) for b, l in enumerate(ids)], voices, list_ids=ids)
    check_apply(plans(4), 4, some, what="four lists shared")


def test_scan_beyond_one_block_of_lengths(base_tables, plans):
    """1,100 utterances (the scan sums 1,024 lengths at a time): room for all, and room that ends inside the second block."""
    table = base_tables["two"]
    points = [cases.make_points(table, 4, 1 + b % 2, "between", 300 + b % 5) for b in range(1100)]
    batch = Batch([table], points, [b % 2 for b in range(1100)], list_ids=[0] * 1100)
    check_apply(plans(4), 4, batch, what="1100")
    _, offsets, _, _ = batch.expected(4, batch.room())
    # utterance 1061 has 4 events, 1062 has 3: the one is dropped, the other takes the last of the room
    _, status = check_apply(plans(4), 4, batch, capacity=int(offsets[1061]) + 3, what="1100, room for 1061 and 3 events")
    assert (status[:1061] == 0).all() and status[1061] == 5 and status[1062] == 0 and (status[1063:] == 5).all()


def test_refused_utterances_between_good_ones(base_tables, plans):
    """Every status, 5 included, between good utterances: the neighbours are unchanged, the refused ones take no room and
    nothing is written beyond out_capacity."""
    hello, two, big = base_tables["hello0"], base_tables["two"], base_tables["r300"]
    empty = np.zeros((0, 38))
    good = lambda t, k: cases.make_points(t, 4, 12, "mix", 400 + k)  # noqa: E731
    bad_time, same_period = good(hello, 1), good(hello, 2)
    bad_time[7, 0] = hello[-1, 0] + 100 + 4 + 0.25   # behind duration + cp
    same_period[5, 0] = same_period[4, 0]            # two points in one control period
    not_finite = good(hello, 3)
    not_finite[0, 0] = np.nan
    too_many = np.zeros((65, 3))
    too_many[:, 0] = 4.0 * np.arange(65)
    lists = [hello, two, empty, big]
    rows = [  # (list, points, voice, status)
        (0, good(hello, 10), SMOOTH, 0),
        (2, good(hello, 11), SMOOTH, 1),          # empty base list
        (0, good(hello, 12), LINEAR, 0),
        (4, good(hello, 13), SMOOTH, 1),          # list id behind the table
        (-1, good(hello, 14), SMOOTH, 1),         # ... and in front of it
        (1, good(two, 15)[:3], SMOOTH, 0),
        (0, good(hello, 16), 2, 1),               # voice id outside the plan's voices
        (0, good(hello, 17), -1, 1),
        (0, too_many, SMOOTH, 2),
        (0, good(hello, 18), SMOOTH, 0),
        (0, bad_time, LINEAR, 3),
        (0, not_finite, LINEAR, 3),
        (1, good(two, 19)[:2], LINEAR, 0),
        (0, same_period, SMOOTH, 4),
        (0, good(hello, 20), SMOOTH, 0),
        (3, cases.make_points(big, 4, 64, "mix", 21), SMOOTH, 5),  # the one that does not fit ...
        (1, good(two, 22)[:1], SMOOTH, 0),                         # ... and a short one behind it that does
        (0, np.zeros((0, 3)), LINEAR, 0),
    ]
    batch = Batch(lists, [r[1] for r in rows], [r[2] for r in rows], list_ids=[r[0] for r in rows])
    # room for every good list but the big one, which would have needed 300 to 364 events
    _, _, _, fits = batch.expected(4, 10 ** 6)
    capacity = sum(len(m) for m, r in zip(fits, rows) if r[3] == 0) + 100
    _, status = check_apply(plans(4), 4, batch, capacity=capacity, what="refused")
    assert status.tolist() == [r[3] for r in rows]
    # with room for all of them the big one is good, and no status is asked for
    _, status = check_apply(plans(4), 4, batch, what="refused, with room")
    assert status.tolist() == [0 if r[3] == 5 else r[3] for r in rows]
    # no room at all: every good utterance is refused, nothing is written
    _, status = check_apply(plans(4), 4, batch, capacity=0, what="no room")
    assert status.tolist() == [5 if r[3] in (0, 5) else r[3] for r in rows]


def singable_contours(table, count, seed):
    """Contours that keep the pitch inside the model's range (track_cases.make_singable: the oscillator must stay inside
    its wavetable for two runs to be comparable at all)."""
    out = contours(table, 4, count, seed)
    rng = np.random.default_rng(seed)
    for p in out:  # points on a gentle curve, with the curve's own slopes: the cubic through them does not overshoot
        phase, rate = rng.uniform(0.0, 6.28), rng.uniform(1 / 400.0, 1 / 150.0)
        p[:, 1] = 3.0 * np.sin(phase + p[:, 0] * rate)
        p[:, 2] = 3.0 * rate * np.cos(phase + p[:, 0] * rate)
    return out


def synthesis_plan(kind):
    if kind == "model5":
        return g.VoicesPlan(configs5(48000.0, names=["male", "female"]), 250.0, 0)
    return g.VoicesPlan(configs(precision=capi.PRECISION_F32 if kind == "f32" else capi.PRECISION_F64, names=["male", "female"]), 250.0, 0)


@pytest.mark.parametrize("kind", ["f32", "f64", "model5"])
def test_one_call_equals_the_separate_calls(base_tables, kind):
    """gvtm_synthesize_intonation_device against gvtm_apply_intonation_device followed by
    gvtm_synthesize_events_voices_device: samples, counts, peaks, frame counts, drift states and statuses, as bytes."""
    plan = synthesis_plan(kind)
    tracks = track_pair(4)
    tracks[LINEAR].mean_pitch = -4.0  # (the female voice's)
    plan.set_voice_tracks(tracks)
    table = base_tables["hello0"]
    points = singable_contours(table, 10, 500)
    points[0][2, 0] = np.inf                    # refused: 3
    points[7] = np.repeat(points[7][:1], 2, 0)  # refused: 4
    voices = [b % 2 for b in range(10)]
    batch = Batch([table], points, voices, list_ids=[0] * 10)
    capacity = batch.room()
    max_frames = max(capi.tracks_frame_count(tracks[v], capi.intonation_apply_host(tracks[v], capi.events_from_table(table), capi.points_from_table(p))[0])
                     for p, v in zip(points, voices))
    stride = plan.voices_output_capacity(max_frames)

    def fresh():
        return dict(audio=filled((10, stride), 0.25, np.float32), frames=filled(10, 99, np.int32), counts=filled(10, 99, np.int64),
                    maxabs=filled(10, 5.0, np.float32), drift=to_device(used_drift(10))[0], status=filled(10, -9, np.int32))

    two, one = fresh(), fresh()
    size = capi.EVENT_DTYPE.itemsize
    d_out, d_offsets = filled(capacity * size, GUARD, np.uint8), filled(11, -7, np.int64)
    plan.apply_intonation_device(batch.d_events, batch.d_list_offsets, 1, batch.d_list_ids, batch.d_points, batch.d_point_offsets, batch.d_voices, 10,
                                 d_out, capacity, d_offsets, two["status"], current_stream())
    plan.synthesize_events_voices_device(d_out, d_offsets, batch.d_voices, 10, max_frames, two["audio"], stride, two["frames"], two["counts"],
                                         two["maxabs"], two["drift"], current_stream())
    plan.synthesize_intonation_device(batch.d_events, batch.d_list_offsets, 1, batch.d_list_ids, batch.d_points, batch.d_point_offsets, batch.d_voices,
                                      capacity, 10, max_frames, one["audio"], stride, one["frames"], one["counts"], one["maxabs"], one["drift"],
                                      one["status"], current_stream())
    two, one = dict(zip(two, to_host(*two.values()))), dict(zip(one, to_host(*one.values())))
    assert two["status"].tolist() == [3, 0, 0, 0, 0, 0, 0, 4, 0, 0]
    good = two["status"] == 0
    assert (two["frames"][good] > 300).all() and (two["frames"][~good] == 0).all() and (two["counts"][good] > 0).all()
    assert two["drift"][~good].tobytes() == used_drift(10)[~good].tobytes()  # a refused utterance leaves its generator alone
    for key in two:
        assert one[key].tobytes() == two[key].tobytes(), (kind, key)
