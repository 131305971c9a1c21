"""Rhythm and intonation-point placement on the device (gvtm_apply_rhythm_device, gvtm_place_intonation_device,
vtm_prosody.hip) against the host entries, which test_prosody_cpu.py holds to the reference: tempi, points, offsets and
statuses bit for bit on every case of prosody_cases.py and on its refusals, in batches of 1, 3 and 65, with and without
draws, with a points buffer too small in the middle; and gvtm_synthesize_prosody_device on a float plan of two voices
against the five calls made one by one, and for the voice without macro intonation against gvtm_synthesize_postures_device.

Outputs start out as a guard pattern and are compared whole, guard included, with the host's results laid out as the device
lays them out."""
import numpy as np
import pytest

import gama_tts_amd as g
from gama_tts_amd import capi
import oracle
import prosody_cases as cases
import rules_cases
from device_io import current_stream, filled, to_device, to_host
from test_prosody_cpu import Prosodies, own, tables, track_config
from test_rules_cpu import as_bits

pytestmark = pytest.mark.gpu

GUARD = 0xA5
GUARD_RECORDS = 8
POINT = capi.POINT_DTYPE.itemsize
POSTURE = capi.POSTURE_DTYPE.itemsize


@pytest.fixture(scope="module")
def golden():
    return np.load(cases.GOLDEN)


@pytest.fixture(scope="module")
def rules():
    made = capi.Rules(dict(np.load(rules_cases.MODEL_0_MALE)), device=0)
    yield made
    made.close()


@pytest.fixture(scope="module")
def prosodies(golden):
    made = Prosodies(golden, device=0)
    yield made
    made.close()


def offsets_of(lists):
    out = np.zeros(len(lists) + 1, dtype=np.int64)
    out[1:] = np.cumsum([len(x) for x in lists])
    return out


def cat(lists, dtype):
    return np.concatenate([np.ascontiguousarray(x, dtype=dtype) for x in lists] + [np.zeros(0, dtype=dtype)])


class Batch:
    """Golden entries and refusals (names of prosody_cases.OWN) as one call's tables, and what the host entries make of them.
    with_draws: the batch has draws, the golden's for an entry the reference drew for, a generator's for every other one."""

    def __init__(self, golden, rules, prosody, names, cp, with_draws=False, max_rules=64):
        self.names, self.cp, self.batch, self.max_rules = names, cp, len(names), max_rules
        rng = np.random.default_rng(len(names))
        self.before, self.feet, self.groups, self.draws = [], [], [], []
        for n in names:
            if n in cases.OWN:
                _, postures, feet, groups, _, _ = own(golden, n)
                draws = None
            else:
                postures, feet, groups, draws = tables(golden, n)
            self.before.append(postures)
            self.feet.append(feet)
            self.groups.append(groups)
            self.draws.append((rng.random((len(feet), 2)) if draws is None else draws) if with_draws else None)
        # the host: rhythm, the rule on its postures, the points
        self.after, self.rhythm_status, self.rule, self.points, self.status = [], [], [], [], []
        for b in range(self.batch):
            after, rhythm_status = prosody.rhythm_host(self.before[b], self.feet[b])
            events, rule_data, onsets, rule_status = rules.apply_host(cp, after)
            if len(rule_data) > max_rules:  # rows the device's table does not hold: refused
                points, status = np.zeros(0, dtype=capi.POINT_DTYPE), capi.PROSODY_NO_RULES
                if capi.prosody_point_count(len(after), self.feet[b], self.groups[b]) < 0:
                    status = capi.PROSODY_BAD_STRUCTURE
            else:
                points, status = prosody.points_host(cp, after, self.feet[b], self.groups[b], self.draws[b], rule_data, onsets, rule_status)
            self.after.append(after)
            self.rhythm_status.append(rhythm_status)
            self.rule.append((events, rule_data, onsets, rule_status))
            self.points.append(points)
            self.status.append(status)
        self.posture_offsets, self.foot_offsets, self.group_offsets = offsets_of(self.before), offsets_of(self.feet), offsets_of(self.groups)
        self.n_postures, self.n_feet = int(self.posture_offsets[-1]), int(self.foot_offsets[-1])
        self.d_posture_offsets, self.d_foot_offsets, self.d_group_offsets = to_device(self.posture_offsets, self.foot_offsets, self.group_offsets)
        self.d_feet, self.d_groups = to_device(as_bits(cat(self.feet, capi.FOOT_DTYPE)), as_bits(cat(self.groups, capi.TONE_GROUP_DTYPE)))
        self.d_draws = to_device(cat([d.reshape(-1) for d in self.draws], np.float64))[0] if with_draws else None

    def room(self):
        return sum(len(p) for p in self.points)

    def expected_points(self, capacity):
        """The host's points laid out as the device lays them out -> (the buffer's bytes, guard included; offsets; statuses)."""
        buf = np.full((capacity + GUARD_RECORDS) * POINT, GUARD, dtype=np.uint8)
        offsets, statuses = np.zeros(self.batch + 1, dtype=np.int64), np.zeros(self.batch, dtype=np.int32)
        at = 0
        for b, (points, status) in enumerate(zip(self.points, self.status)):
            if status == 0 and at + len(points) > capacity:
                points, status = points[:0], capi.PROSODY_NO_ROOM
            buf[at * POINT: (at + len(points)) * POINT] = as_bits(points)
            at += len(points)
            offsets[b + 1], statuses[b] = at, status
        return buf, offsets, statuses

    def rule_tables(self):
        """What gvtm_generate_events_device would have left of the host's rule: (rule data [batch][max_rules], counts, onsets, statuses)"""
        rows = np.zeros((self.batch, self.max_rules), dtype=capi.RULE_DATA_DTYPE)
        for b, (_, rule_data, _, _) in enumerate(self.rule):
            kept = min(len(rule_data), self.max_rules)
            rows[b, :kept] = rule_data[:kept]
        counts = np.asarray([len(r[1]) for r in self.rule], dtype=np.int32)
        return as_bits(rows), counts, cat([r[2] for r in self.rule], np.float64), np.asarray([r[3] for r in self.rule], dtype=np.int32)

    def place(self, prosody, capacity):
        d_after, = to_device(as_bits(cat(self.after, capi.POSTURE_DTYPE)))
        d_rows, d_counts, d_onsets, d_status = to_device(*self.rule_tables())
        d_points, d_offsets = filled((capacity + GUARD_RECORDS) * POINT, GUARD, np.uint8), filled(self.batch + 1, -7, np.int64)
        prosody.place_intonation_device(self.cp, d_after, self.d_posture_offsets, self.d_feet, self.d_foot_offsets, self.d_groups, self.d_group_offsets,
                                        self.d_draws, self.batch, d_rows, self.max_rules, d_counts, d_onsets, d_points, capacity, d_offsets, d_status,
                                        current_stream())
        return to_host(d_points, d_offsets, d_status)


def check_points(batch, prosody, capacity=None, what=""):
    capacity = batch.room() if capacity is None else capacity
    want_buf, want_off, want_status = batch.expected_points(capacity)
    got_buf, got_off, got_status = batch.place(prosody, capacity)
    assert np.array_equal(got_status, want_status), (what, got_status.tolist(), want_status.tolist())
    assert np.array_equal(got_off, want_off), (what, got_off.tolist(), want_off.tolist())
    if not np.array_equal(got_buf, want_buf):
        bad = np.flatnonzero(got_buf != want_buf)
        point, byte = divmod(int(bad[0]), POINT)
        raise AssertionError("%s: %d bytes differ, first in point %d of the output (capacity %d) at byte %d" % (what, bad.size, point, capacity, byte))
    return want_status


def check_rhythm(batch, prosody, in_place, what=""):
    before = as_bits(cat(batch.before, capi.POSTURE_DTYPE))
    d_in = filled((batch.n_postures + GUARD_RECORDS) * POSTURE, GUARD, np.uint8)
    d_in[: before.size] = to_device(before)[0]
    d_out = d_in if in_place else filled((batch.n_postures + GUARD_RECORDS) * POSTURE, GUARD, np.uint8)
    d_status = filled(batch.batch, -9, np.int32)
    prosody.apply_rhythm_device(d_in, batch.d_posture_offsets, batch.n_postures, batch.d_feet, batch.d_foot_offsets, batch.n_feet, batch.batch, d_out, d_status,
                                current_stream())
    got_in, got, status = to_host(d_in, d_out, d_status)
    assert status.tolist() == batch.rhythm_status, (what, status.tolist(), batch.rhythm_status)
    assert (got[batch.n_postures * POSTURE:] == GUARD).all(), what
    if not in_place:
        assert np.array_equal(got_in[: before.size], before), what
    for b in range(batch.batch):  # (the tempi of a refused utterance are not defined)
        if batch.rhythm_status[b] == 0:
            lo, hi = batch.posture_offsets[b] * POSTURE, batch.posture_offsets[b + 1] * POSTURE
            assert np.array_equal(got[lo:hi], as_bits(batch.after[b])), (what, b, batch.names[b])


def groups_of_entries(golden):
    """The golden entries by what one call shares: the control period and the prosody object."""
    found = {}
    for n in cases.entry_names(golden):
        found.setdefault((int(golden[n + "__cp"]), float(golden[n + "__intonation_factor"]), float(golden[n + "__global_tempo"])), []).append(n)
    return found


GROUPS = groups_of_entries(np.load(cases.GOLDEN))


def pool(golden):
    """The entries under cp 4 and the files' two factors, and every refusal: what the batches are drawn from"""
    return GROUPS[(4, 1.0, 1.0)] + sorted(cases.OWN)


@pytest.mark.parametrize("key", sorted(GROUPS), ids=lambda k: "cp%d-factor%g-tempo%g" % k)
@pytest.mark.parametrize("with_draws", [False, True], ids=["plain", "draws"])
def test_every_case_on_the_device(golden, rules, prosodies, key, with_draws):
    names = GROUPS[key] + (sorted(cases.OWN) if key[0] == 4 else [])
    prosody = prosodies.of(GROUPS[key][0])
    batch = Batch(golden, rules, prosody, names, key[0], with_draws)
    statuses = check_points(batch, prosody, what=str(key))
    assert (statuses[: len(GROUPS[key])] == 0).all()
    for in_place in (False, True):
        check_rhythm(batch, prosody, in_place, what=str(key))


@pytest.mark.parametrize("size", [1, 3, 65])
@pytest.mark.parametrize("with_draws", [False, True], ids=["plain", "draws"])
def test_batches(golden, rules, prosodies, size, with_draws):
    names = [pool(golden)[(5 * size + 7 * b) % len(pool(golden))] for b in range(size)]
    prosody = prosodies.of("hello.0")
    batch = Batch(golden, rules, prosody, names, 4, with_draws, max_rules=36 if size == 65 else 64)
    statuses = check_points(batch, prosody, what="batch %d" % size)
    if size == 65:  # refused utterances among good ones, the sentence's 37 rule rows among them
        assert set(statuses.tolist()) >= {0, 1, 2, 3}
    check_rhythm(batch, prosody, size != 3, what="batch %d" % size)
    if size == 65:
        assert set(batch.rhythm_status) == {0, 1, 4}


def test_points_that_do_not_fit_in_the_middle(golden, rules, prosodies):
    names = ["one_tonic", "hello.0", "points_64", "two_groups", "points_65", "delta_zero"]
    prosody = prosodies.of("hello.0")
    batch = Batch(golden, rules, prosody, names, 4)
    capacity = batch.room() - 64 + 9  # the 64 points do not fit; the 7 and the 5 behind them do
    statuses = check_points(batch, prosody, capacity=capacity, what="overflow")
    assert statuses.tolist() == [0, 0, 5, 0, 3, 0]
    assert (check_points(batch, prosody, capacity=0, what="no room at all")[[0, 1, 2, 3, 5]] == 5).all()


def test_the_chain_step_by_step_against_the_prosody_entry(golden, rules, prosodies):
    """Two male voices on a float plan, the second without macro intonation.  hello.0 under either voice, a case with draws,
    65 points (refused by the placement) and two postures the rule refuses (no feet, no groups)."""
    prosody = prosodies.of("hello.0")
    names = ["hello.0", "random_1", "hello.0", "points_65", "one_tonic"]
    voices = np.asarray([0, 0, 1, 0, 0], dtype=np.int32)
    batch = Batch(golden, rules, prosody, names, 4, with_draws=True)
    # (the last utterance: two postures at sixty times the tempo, "the time interval between two postures is too small")
    small = np.load(rules_cases.GOLDEN)
    batch.before[4] = capi.postures_from_table(rules_cases.posture_records(small, "m_small_di"))
    batch.feet[4], batch.groups[4], batch.draws[4] = batch.feet[4][:0], batch.groups[4][:0], batch.draws[4][:0]
    posture_offsets, foot_offsets, group_offsets = offsets_of(batch.before), offsets_of(batch.feet), offsets_of(batch.groups)
    n_postures, n_feet, size = int(posture_offsets[-1]), int(foot_offsets[-1]), len(names)
    d_before, d_feet, d_groups, d_draws, d_voices = to_device(as_bits(cat(batch.before, capi.POSTURE_DTYPE)), as_bits(cat(batch.feet, capi.FOOT_DTYPE)),
                                                              as_bits(cat(batch.groups, capi.TONE_GROUP_DTYPE)),
                                                              cat([d.reshape(-1) for d in batch.draws], np.float64), voices)
    d_po, d_fo, d_go = to_device(posture_offsets, foot_offsets, group_offsets)
    # the step-by-step caller leaves the groups of the voice without macro intonation out
    quiet = [gr[:0] if voices[b] == 1 else gr for b, gr in enumerate(batch.groups)]
    d_quiet_groups, d_quiet_go = to_device(as_bits(cat(quiet, capi.TONE_GROUP_DTYPE)), offsets_of(quiet))

    config = g.config_from_dict(g.read_config_file(oracle.VOICE_MALE), 44100.0, 1, capi.PRECISION_F32)
    plan = g.VoicesPlan([config, config], 250.0, 0)
    plan.set_voice_tracks([track_config(4, macro=1), track_config(4, macro=0)])
    # sizes from the host: the lists the rule makes of the postures after rhythm, and what the points add
    lists = []
    for b in range(size):
        after, _ = prosody.rhythm_host(batch.before[b], batch.feet[b])
        lists.append(rules.apply_host(4, after)[0])
    events_capacity, points_capacity, max_rules = sum(len(e) for e in lists), 2 * capi.MAX_INTONATION_POINTS, 40
    merged0 = capi.intonation_apply_host(track_config(4), lists[0], batch.points[0])[0]
    max_frames = max(capi.tracks_frame_count(track_config(4), e) for e in lists + [merged0] if len(e)) + 8
    stride = plan.voices_output_capacity(max_frames)

    def outputs():
        return [filled((size, stride), 0.0, np.float32), filled(size, 99, np.int32), filled(size, 99, np.int64), filled(size, 5.0, np.float32),
                filled(size, -9, np.int32), filled(size, -9, np.int32)]

    stream = current_stream()
    want = outputs()
    d_after, d_rhythm_status = filled(n_postures * POSTURE, GUARD, np.uint8), filled(size, -9, np.int32)
    prosody.apply_rhythm_device(d_before, d_po, n_postures, d_feet, d_fo, n_feet, size, d_after, d_rhythm_status, stream)
    d_gen, d_gen_off = filled(events_capacity * capi.EVENT_DTYPE.itemsize, GUARD, np.uint8), filled(size + 1, -7, np.int64)
    d_rows, d_counts, d_onsets = filled(size * max_rules * capi.RULE_DATA_DTYPE.itemsize, GUARD, np.uint8), filled(size, -3, np.int32), filled(n_postures, -1.0, np.float64)
    rules.generate_events_device(4, d_after, d_po, size, d_gen, events_capacity, d_gen_off, d_rows, max_rules, d_counts, d_onsets, want[4], stream)
    d_points, d_point_off = filled(points_capacity * POINT, GUARD, np.uint8), filled(size + 1, -7, np.int64)
    prosody.place_intonation_device(4, d_after, d_po, d_feet, d_fo, d_quiet_groups, d_quiet_go, d_draws, size, d_rows, max_rules, d_counts, d_onsets, d_points,
                                    points_capacity, d_point_off, want[4], stream)
    prosody_status = to_host(want[4])[0]
    assert prosody_status.tolist() == [0, 0, 0, 3, 2] and to_host(d_rhythm_status)[0].tolist() == [0] * size
    d_list_ids, = to_device(np.where(prosody_status == 0, np.arange(size), -1).astype(np.int32))
    merged_capacity = events_capacity + points_capacity
    d_merged, d_merged_off = filled(merged_capacity * capi.EVENT_DTYPE.itemsize, GUARD, np.uint8), filled(size + 1, -7, np.int64)
    plan.apply_intonation_device(d_gen, d_gen_off, size, d_list_ids, d_points, d_point_off, d_voices, size, d_merged, merged_capacity, d_merged_off, want[5], stream)
    plan.synthesize_events_voices_device(d_merged, d_merged_off, d_voices, size, max_frames, want[0], stride, want[1], want[2], want[3], None, stream)

    got = outputs()
    plan.synthesize_prosody_device(rules, prosody, d_before, d_po, n_postures, d_feet, d_fo, n_feet, d_groups, d_go, d_draws, d_voices, max_rules, points_capacity,
                                   events_capacity, size, max_frames, got[0], stride, got[1], got[2], got[3], None, got[4], got[5], stream)
    want, got = to_host(*want), to_host(*got)
    assert want[4].tolist() == [0, 0, 0, 3, 2] and want[5].tolist() == [0, 0, 0, 1, 1]
    assert (want[1][:3] > 0).all() and (want[1][3:] == 0).all() and (want[2][:3] > 0).all() and np.abs(want[0][:3]).max() > 0
    assert not np.array_equal(want[0][0], want[0][2])  # the contour is heard
    for w, h in zip(want, got):
        assert np.array_equal(as_bits(w), as_bits(h))

    # the voice without macro intonation: gvtm_synthesize_postures_device's samples on the postures after rhythm
    single = g.Plan(config, 250.0, 0)
    after, _ = prosody.rhythm_host(batch.before[2], batch.feet[2])
    d_one, d_one_off = to_device(as_bits(after), np.asarray([0, len(after)], dtype=np.int64))
    one_stride = single.output_count(max_frames)
    d_audio, d_frames, d_samples = filled((1, one_stride), 0.0, np.float32), filled(1, 99, np.int32), filled(1, 99, np.int64)
    single.synthesize_postures_device(rules, track_config(4, macro=0), d_one, d_one_off, len(lists[2]), 1, max_frames, d_audio, one_stride, d_frames, d_samples,
                                      None, None, None, stream)
    audio, frames, samples = to_host(d_audio, d_frames, d_samples)
    assert frames[0] == got[1][2] and samples[0] == got[2][2]
    assert np.array_equal(audio[0, : samples[0]].view(np.uint32), got[0][2, : samples[0]].view(np.uint32))
    single.close()
    plan.close()
