"""Event lists from posture sequences on the device (gvtm_generate_events_device, vtm_rules.hip): lists, offsets, rule data,
onsets and statuses bit for bit gvtm_rules_apply_host's and the reference's (tests/golden/rules_golden.npz) on every case of
rules_cases.py, in batches of 1, 3 and 65 with refused utterances among good ones and one list that does not fit; the same
with the optional outputs NULL; gvtm_synthesize_postures_device on a float plan against gvtm_synthesize_events_device fed the
reference's lists; and the generated lists under the intonation fixture's points against the reference's lists under them.

Lists are compared as bytes.  The event buffer starts out as a guard pattern, and the whole buffer -- the lists' room, the
refused utterances' none, GUARD_EVENTS events behind out_capacity -- is compared with the pattern laid out on the host."""
import numpy as np
import pytest

import gama_tts_amd as g
from gama_tts_amd import capi
import intonation_cases
import oracle
import rules_cases as cases
from device_io import current_stream, filled, to_device, to_host
from test_rules_cpu import as_bits, golden_events, golden_rule_data

pytestmark = pytest.mark.gpu

GUARD = 0xA5
GUARD_EVENTS = 8
EVENT = capi.EVENT_DTYPE.itemsize


@pytest.fixture(scope="module")
def golden():
    return np.load(cases.GOLDEN)


@pytest.fixture(scope="module")
def rules(golden):
    made = {m: capi.Rules(cases.model_arrays(golden, m), device=0) for m in cases.MODELS}
    yield made
    for r in made.values():
        r.close()


class Batch:
    """Golden entries of one model as one call's postures, on the device, and what the host rule makes of them."""

    def __init__(self, golden, rules, names, cp):
        self.names, self.cp, self.batch = names, cp, len(names)
        self.postures = [capi.postures_from_table(cases.posture_records(golden, n)) for n in names]
        self.offsets = np.zeros(self.batch + 1, dtype=np.int64)
        self.offsets[1:] = np.cumsum([len(p) for p in self.postures])
        self.d_postures, self.d_offsets = to_device(np.concatenate(self.postures).view(np.uint8), self.offsets)
        self.host = [rules.apply_host(cp, p) for p in self.postures]  # (events, rule data, onsets, status)
        for n, (events, _, _, status) in zip(names, self.host):  # the host rule is the reference's (test_rules_cpu.py), once more
            assert status == cases.expected_status(golden, n) and np.array_equal(as_bits(events), as_bits(golden_events(golden, n))), n

    def room(self):
        return sum(len(h[0]) for h in self.host)

    def expected(self, capacity):
        """The host's lists laid out as the device lays them out -> (the event buffer's bytes, guard included; offsets; statuses)."""
        buf = np.full((capacity + GUARD_EVENTS) * EVENT, GUARD, dtype=np.uint8)
        offsets, statuses = np.zeros(self.batch + 1, dtype=np.int64), np.zeros(self.batch, dtype=np.int32)
        at = 0
        for b, (events, _, _, status) in enumerate(self.host):
            if status == 0 and at + len(events) > capacity:
                events, status = events[:0], 5
            buf[at * EVENT: (at + len(events)) * EVENT] = events.view(np.uint8)
            at += len(events)
            offsets[b + 1], statuses[b] = at, status
        return buf, offsets, statuses

    def generate(self, rules, capacity, max_rules=None):
        """gvtm_generate_events_device into guarded buffers; max_rules None: the optional outputs NULL."""
        d_out = filled((capacity + GUARD_EVENTS) * EVENT, GUARD, np.uint8)
        d_off, d_status = filled(self.batch + 1, -7, np.int64), filled(self.batch, -9, np.int32)
        if max_rules is None:
            rules.generate_events_device(self.cp, self.d_postures, self.d_offsets, self.batch, d_out, capacity, d_off, None, 0, None, None, None, current_stream())
            return to_host(d_out, d_off)
        d_rule = filled(self.batch * max_rules * capi.RULE_DATA_DTYPE.itemsize, GUARD, np.uint8)
        d_counts, d_onsets = filled(self.batch, -3, np.int32), filled(int(self.offsets[-1]), -1.0, np.float64)
        rules.generate_events_device(self.cp, self.d_postures, self.d_offsets, self.batch, d_out, capacity, d_off, d_rule, max_rules, d_counts, d_onsets,
                                     d_status, current_stream())
        return to_host(d_out, d_off, d_status, d_rule, d_counts, d_onsets)


def check(golden, rules, names, cp, capacity=None, max_rules=64, what=""):
    batch = Batch(golden, rules, names, cp)
    capacity = batch.room() if capacity is None else capacity
    want_buf, want_off, want_status = batch.expected(capacity)
    got_buf, got_off, got_status, got_rule, got_counts, got_onsets = batch.generate(rules, capacity, max_rules)
    assert np.array_equal(got_status, want_status), (what, got_status.tolist(), want_status.tolist())
    assert np.array_equal(got_off, want_off), (what, got_off.tolist(), want_off.tolist())
    if not np.array_equal(got_buf, want_buf):
        bad = np.flatnonzero(got_buf != want_buf)
        event, byte = divmod(int(bad[0]), EVENT)
        raise AssertionError("%s: %d bytes differ, first in event %d of the output (capacity %d) at byte %d" % (what, bad.size, event, capacity, byte))
    row = capi.RULE_DATA_DTYPE.itemsize
    got_rule = got_rule.reshape(batch.batch, max_rules * row)
    for b, (_, rule_data, onsets, status) in enumerate(batch.host):
        # (status 5 is the scan's: the count kernel had accepted the utterance, its rule data and onsets stand)
        assert got_counts[b] == (len(rule_data) if want_status[b] in (0, 5) else 0), (what, b)
        if status == 0:
            kept = min(len(rule_data), max_rules)
            assert np.array_equal(got_rule[b, : kept * row], as_bits(rule_data[:kept])), (what, b)
            assert (got_rule[b, kept * row:] == GUARD).all(), (what, b)
            assert np.array_equal(got_onsets[batch.offsets[b]: batch.offsets[b + 1]].view(np.uint64), onsets.view(np.uint64)), (what, b)
    # the optional outputs NULL: the same lists and offsets
    null_buf, null_off = batch.generate(rules, capacity)
    assert np.array_equal(null_off, want_off) and np.array_equal(null_buf, want_buf), what
    return batch, want_status


@pytest.mark.parametrize("model,cp", [(m, cp) for m in cases.MODELS for cp in (1, 2, 3, 4)])
def test_every_case_on_the_device(golden, rules, model, cp):
    names = cases.entries_of(golden, model, cp)
    assert names
    check(golden, rules[model], names, cp, what="%s cp %d" % (model, cp))


@pytest.mark.parametrize("size", [1, 3, 65])
@pytest.mark.parametrize("model", cases.MODELS)
def test_batches(golden, rules, model, size):
    pool = cases.entries_of(golden, model, 4)
    names = [pool[(7 * size + 3 * b) % len(pool)] for b in range(size)]
    _, statuses = check(golden, rules[model], names, 4, max_rules=5, what="%s batch %d" % (model, size))
    if size == 65:
        assert (statuses == 0).any() and len(set(statuses.tolist())) >= 3  # refused utterances among good ones


def test_a_list_in_the_middle_does_not_fit(golden, rules):
    names = ["m_two", "hello.0", "sentence.0", "m_three", "m_small_di", "m_four"]
    batch = Batch(golden, rules["0_male"], names, 4)
    capacity = batch.room() - len(batch.host[2][0]) + 5  # the sentence does not fit; the three short lists behind it do
    _, statuses = check(golden, rules["0_male"], names, 4, capacity=capacity, what="overflow")
    assert statuses.tolist() == [0, 0, 5, 0, 2, 0]
    check(golden, rules["0_male"], names, 4, capacity=0, what="no room at all")


def test_the_longest_list_passes_the_tracks_kernels_table(golden, rules):
    """The sentence's list is longer than the 240 events the tracks kernel keeps in LDS at a time: its frames on the generated
    list are the frames on the reference's list."""
    batch = Batch(golden, rules["0_male"], ["sentence.0"], 4)
    want = golden_events(golden, "sentence.0")
    assert len(want) > 240
    config = capi.TrackConfig(control_period_ms=4, macro_intonation=0, micro_intonation=1, intonation_drift=0, smooth_intonation=1,
                              initial_pitch=0.0, mean_pitch=-12.0, drift_deviation=1.0, drift_sample_rate=250.0, drift_lowpass_cutoff=4.0)
    max_frames = capi.tracks_frame_count(config, want)
    d_out, d_off = filled(len(want) * EVENT, GUARD, np.uint8), filled(2, -7, np.int64)
    rules["0_male"].generate_events_device(4, batch.d_postures, batch.d_offsets, 1, d_out, len(want), d_off, stream=current_stream())
    frames = []
    for d_events, d_offsets in ((d_out, d_off), to_device(want.view(np.uint8), np.array([0, len(want)], dtype=np.int64))):
        d_params, d_counts = filled((1, max_frames, 16), 7.0, np.float32), filled(1, 99, np.int32)
        capi.generate_tracks_device(config, d_events, d_offsets, 1, max_frames, d_params, d_counts, None, current_stream())
        frames.append(to_host(d_params, d_counts))
    assert frames[0][1][0] == frames[1][1][0] == max_frames
    assert np.array_equal(frames[0][0].view(np.uint32), frames[1][0].view(np.uint32))


def test_postures_to_samples_on_a_float_plan(golden, rules):
    """gvtm_synthesize_postures_device against gvtm_synthesize_events_device fed the reference's lists: samples, counts,
    peaks and frame counts bit for bit."""
    names = ["m_two", "hello.0", "m_small_di"]
    batch = Batch(golden, rules["0_male"], names, 4)
    lists = [golden_events(golden, n) for n in names]
    plan = g.Plan(g.config_from_dict(g.read_config_file(oracle.VOICE_MALE), 44100.0, 1, capi.PRECISION_F32), 250.0, 0)
    config = capi.TrackConfig(control_period_ms=4, macro_intonation=0, micro_intonation=1, intonation_drift=1, smooth_intonation=1,
                              initial_pitch=0.0, mean_pitch=-12.0, drift_deviation=1.0, drift_sample_rate=250.0, drift_lowpass_cutoff=4.0)
    max_frames = max(capi.tracks_frame_count(config, e) for e in lists if len(e))
    stride = plan.output_count(max_frames)
    offsets = np.zeros(len(lists) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(e) for e in lists])
    d_events, d_offsets = to_device(np.concatenate(lists).view(np.uint8), offsets)

    def outputs():
        return [filled((len(names), stride), 0.0, np.float32), filled(len(names), 99, np.int32), filled(len(names), 99, np.int64),
                filled(len(names), 5.0, np.float32)]

    want, got = outputs(), outputs()
    plan.synthesize_events_device(config, d_events, d_offsets, len(names), max_frames, want[0], stride, want[1], want[2], want[3], None, current_stream())
    d_status = filled(len(names), -9, np.int32)
    plan.synthesize_postures_device(rules["0_male"], config, batch.d_postures, batch.d_offsets, batch.room(), len(names), max_frames, got[0], stride,
                                    got[1], got[2], got[3], None, d_status, current_stream())
    want, got, status = to_host(*want), to_host(*got), to_host(d_status)[0]
    assert status.tolist() == [0, 0, 2]
    assert want[1].tolist()[:2] == [capi.tracks_frame_count(config, e) for e in lists[:2]] and want[1][2] == 0
    assert (want[2][:2] > 0).all() and np.abs(want[0][:2]).max() > 0
    for w, h in zip(want, got):
        assert np.array_equal(w.view(np.uint8) if w.dtype.kind == "f" else w, h.view(np.uint8) if h.dtype.kind == "f" else h)
    plan.close()


def test_generated_lists_under_the_intonation_fixtures_points(golden, rules, golden_tracks):
    """The device's lists go straight to gvtm_apply_intonation_device: merged lists, offsets and statuses are those the entry
    gives on the reference's lists, uploaded, under the same points."""
    names = ["hello.0", "m_four", "sentence.0"]
    batch = Batch(golden, rules["0_male"], names, 4)
    base_tables = intonation_cases.bases(golden_tracks)
    points = [intonation_cases.case(n, base_tables)[1] for n in ("hello0_p12", "hello0_p2_on", "hello0_p64")]
    point_offsets = np.zeros(len(points) + 1, dtype=np.int64)
    point_offsets[1:] = np.cumsum([len(p) for p in points])
    d_points, d_point_offsets, d_voices = to_device(np.concatenate(points), point_offsets, np.zeros(len(names), dtype=np.int32))
    plan = g.VoicesPlan([g.config_from_dict(g.read_config_file(oracle.VOICE_MALE), 44100.0, 1)], 250.0, 0)
    plan.set_voice_tracks([capi.TrackConfig(control_period_ms=4, macro_intonation=1, micro_intonation=1, intonation_drift=0, smooth_intonation=1,
                                            initial_pitch=0.0, mean_pitch=-12.0, drift_deviation=1.0, drift_sample_rate=250.0, drift_lowpass_cutoff=4.0)])
    d_gen, d_gen_off = filled(batch.room() * EVENT, GUARD, np.uint8), filled(len(names) + 1, -7, np.int64)
    rules["0_male"].generate_events_device(4, batch.d_postures, batch.d_offsets, len(names), d_gen, batch.room(), d_gen_off, stream=current_stream())
    lists = [golden_events(golden, n) for n in names]
    offsets = np.zeros(len(lists) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(e) for e in lists])
    capacity = int(offsets[-1] + point_offsets[-1])
    merged = []
    for d_events, d_offsets in ((d_gen, d_gen_off), to_device(np.concatenate(lists).view(np.uint8), offsets)):
        d_out, d_off, d_status = filled((capacity + GUARD_EVENTS) * EVENT, GUARD, np.uint8), filled(len(names) + 1, -7, np.int64), filled(len(names), -9, np.int32)
        plan.apply_intonation_device(d_events, d_offsets, len(names), None, d_points, d_point_offsets, d_voices, len(names), d_out, capacity, d_off, d_status,
                                     current_stream())
        merged.append(to_host(d_out, d_off, d_status))
    assert 0 in merged[1][2].tolist() and merged[1][1][-1] > offsets[-1]
    for a, b in zip(*merged):
        assert np.array_equal(a, b)
    plan.close()
