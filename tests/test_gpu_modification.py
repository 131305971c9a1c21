"""Parameter-modification gestures applied to frames on the device (gvtm_apply_modifications_device, vtm_modification.hip):
frames, frame counts and statuses bit for bit gvtm_modification_apply_host's, in batches of 1, 2, 3 and 67 over shared bases
of 2, 3, 17 and 40 frames and over a base per utterance, under two voices that differ in control steps and filter length,
with 0 to 5 gestures per utterance from the case table, one utterance of 64 gestures and one of 65, and a refused utterance
of every status between good ones; the one-call entry (gvtm_synthesize_modified_device) against the calls made separately;
the device's audio on host-rule frames against the oracle; and frames-level parity on a one-voice plan and on both classes
of model 5, whose filter is three times as long.

Everything is compared as bytes.  The output buffers start out as a guard pattern, and the whole buffer -- the rows' first F
frames, the rest of every row, the refused utterances' whole rows -- is compared with the pattern laid out on the host, so
anything written where nothing should be shows."""
import numpy as np
import pytest

import gama_tts_amd as g
from gama_tts_amd import capi
import modification_cases as cases
import oracle
import tracks
from device_io import current_stream, filled, to_device, to_host
from parity_rules import check_batch
from voice_cases import configs, oracle_config

pytestmark = pytest.mark.gpu

GUARD = 0xA5       # every byte of an output buffer before the call
MAX_FRAMES = 40
VOICE_KEYS = ("male", "female")  # voice v of the two-voice plan is PLANS[VOICE_KEYS[v]]
ADD, MULTIPLY, R3, FRIC_VOL, VELUM = cases.ADD, cases.MULTIPLY, cases.R3, cases.FRIC_VOL, cases.VELUM


@pytest.fixture(scope="module")
def plan():
    p = g.VoicesPlan(configs(44100.0, 1, capi.PRECISION_F32, names=list(VOICE_KEYS)), 250.0, 0)
    for v, key in enumerate(VOICE_KEYS):
        info = p.voice_info(v)
        assert (info.internal_rate_hz, info.control_steps) == tuple(cases.PLANS[key])
    return p


def pool(key):
    """The gestures of the case table made for plan `key`, one list: utterances draw from it."""
    return [gesture for name, c in cases.CASES.items() if c[0] == key and len(c[3]) < 10 for gesture in c[3]]


class Batch:
    """Bases (float32 [F][16] each), per utterance its base, gestures and voice; on the device as the entries take them.
    voices None: null voice ids.  doctor(tables): a change to the packed tables (what the host entry cannot be given);
    status_of[b]: the status such an utterance must get."""

    def __init__(self, bases, gestures, voices, base_ids=None, max_frames=MAX_FRAMES, doctor=None, status_of=None):
        self.bases, self.gestures, self.voices, self.base_ids = bases, gestures, voices, base_ids
        self.batch, self.max_frames, self.status_of = len(gestures), max_frames, status_of or {}
        rows = np.full((len(bases), max_frames, 16), 9.5, dtype=np.float32)  # (behind a base's frames: never read)
        for l, base in enumerate(bases):
            rows[l, : min(base.shape[0], max_frames)] = base[:max_frames]
        self.tables = dict(zip(("gestures", "gesture_offsets", "utt_gestures", "steps", "values"), capi.pack_gestures(gestures)))
        if doctor:
            doctor(self.tables)
        t = self.tables
        # (no table is empty on the device: one spare entry each)
        self.d_rows, self.d_counts, self.d_gestures, self.d_gesture_offsets, self.d_utt, self.d_steps, self.d_values = to_device(
            rows, np.array([b.shape[0] for b in bases], dtype=np.int32), np.concatenate([t["gestures"], np.zeros((1, 2), np.int32)]), t["gesture_offsets"],
            t["utt_gestures"], np.concatenate([t["steps"], np.zeros(1, np.int32)]), np.concatenate([t["values"], np.zeros(1, np.float32)]))
        self.d_base_ids = None if base_ids is None else to_device(np.asarray(base_ids, dtype=np.int32))[0]
        self.d_voices = None if voices is None else to_device(np.asarray(voices, dtype=np.int32))[0]

    def inputs(self):
        return (self.d_rows, self.d_counts, len(self.bases), self.d_base_ids, self.d_gestures, self.d_gesture_offsets, self.d_utt, self.d_steps,
                self.d_values, self.d_voices, self.batch, self.max_frames)

    def expected(self, plan, n_voices):
        """The host entry utterance by utterance, laid out as the device lays the rows out -> (the output buffer's bytes,
        guard included; frame counts; statuses; the frames of the good utterances)."""
        buf = np.full((self.batch, self.max_frames * 64), GUARD, dtype=np.uint8)
        counts, statuses, frames = np.zeros(self.batch, np.int32), np.zeros(self.batch, np.int32), {}
        for b in range(self.batch):
            l = b if self.base_ids is None else int(self.base_ids[b])
            v = 0 if self.voices is None else int(self.voices[b])
            if b in self.status_of:
                statuses[b] = self.status_of[b]
            elif not (0 <= l < len(self.bases) and 0 <= v < n_voices) or self.bases[l].shape[0] > self.max_frames:
                statuses[b] = 1
            else:
                out, statuses[b] = capi.modification_apply_host(plan, self.bases[l], self.gestures[b], voice=v)
                if statuses[b] == 0:
                    counts[b] = out.shape[0]
                    buf[b, : out.size * 4] = out.view(np.uint8).reshape(-1)
                    frames[b] = out
        return buf, counts, statuses, frames

    def apply(self, plan, status=True):
        d_out = filled((self.batch, self.max_frames * 64), GUARD, np.uint8)
        d_counts, d_status = filled(self.batch, -7, np.int32), filled(self.batch, -9, np.int32)
        plan.apply_modifications_device(*self.inputs(), d_out, d_counts, d_status if status else None, current_stream())
        return d_out, d_counts, d_status


def check_apply(plan, batch, n_voices=2, what=""):
    want_buf, want_counts, want_status, frames = batch.expected(plan, n_voices)
    got_buf, got_counts, got_status = to_host(*batch.apply(plan))
    assert np.array_equal(got_status, want_status), (what, got_status.tolist(), want_status.tolist())
    assert np.array_equal(got_counts, want_counts), (what, got_counts.tolist(), want_counts.tolist())
    if not np.array_equal(got_buf, want_buf):
        bad = np.argwhere(got_buf != want_buf)
        raise AssertionError("%s: %d bytes differ, first in utterance %d, frame %d, parameter %d" %
                             (what, bad.shape[0], bad[0][0], bad[0][1] // 64, bad[0][1] % 64 // 4))
    return want_status, frames


def shared_bases():
    return [cases.base_frames(f, 300 + f) for f in (2, 3, 17, 40)]


def drawn(size, seed):
    """`size` utterances: voices in turn, 0 to 5 gestures each from the pool of the utterance's voice."""
    rng = np.random.default_rng([seed, size])
    pools = [pool(key) for key in VOICE_KEYS]
    voices = [(b + seed) % 2 for b in range(size)]
    gestures = [[pools[v][i] for i in rng.choice(len(pools[v]), (b + seed) % 6, replace=False)] for b, v in enumerate(voices)]
    return gestures, voices


@pytest.mark.parametrize("size", [1, 2, 3, 67])
def test_batches_over_shared_bases_and_over_bases_of_their_own(plan, size):
    gestures, voices = drawn(size, 3)
    if size == 67:
        many = cases.CASES["male__g64"][3]
        gestures[20], voices[20] = many, 0
        gestures[41], voices[41] = many + many[:1], 0   # 65: refused
        gestures[42], voices[42] = many, 1              # (the male case's steps under the female voice: another cs and N)
    bases = shared_bases()
    ids = [(7 * b + 3) % 4 for b in range(size)]
    status, _ = check_apply(plan, Batch(bases, gestures, voices, base_ids=ids), what="shared, batch %d" % size)
    assert status.tolist() == [2 if size == 67 and b == 41 else 0 for b in range(size)]
    # a base per utterance, null ids: the same bytes
    own = Batch([bases[i] for i in ids], gestures, voices)
    check_apply(plan, own, what="own bases, batch %d" % size)
    assert to_host(own.apply(plan)[0])[0].tobytes() == to_host(Batch(bases, gestures, voices, base_ids=ids).apply(plan)[0])[0].tobytes()
    # no status asked for
    got = to_host(*own.apply(plan, status=False))
    assert (got[2] == -9).all() and got[0].tobytes() == own.expected(plan, 2)[0].tobytes()


def test_every_case_of_the_two_voices_against_the_fixture(plan):
    """The cases of the case table made for the two voices, one batch: the device's frames are the reference's."""
    fixture = dict(np.load(oracle.GOLDEN_DIR + "/modification_golden.npz", allow_pickle=False))
    names = [n for n, c in cases.CASES.items() if c[0] in VOICE_KEYS]
    inputs = [cases.case(n) for n in names]
    batch = Batch([base for _, base, _ in inputs], [gs for _, _, gs in inputs], [VOICE_KEYS.index(key) for key, _, _ in inputs])
    status, frames = check_apply(plan, batch, what="fixture cases")
    assert (status == 0).all()
    for b, n in enumerate(names):
        assert cases.check_frames(fixture, n, frames[b]) is None


def test_refused_utterances_between_good_ones(plan):
    bases = shared_bases() + [cases.base_frames(1, 1), cases.base_frames(0, 2), cases.base_frames(41, 3)]
    both = pool("male") + pool("female")
    good = lambda k: [both[i] for i in np.random.default_rng(k).choice(len(both), 5, replace=False)]  # noqa: E731
    point = lambda step, value=0.5: ([step], np.float32([value]))  # noqa: E731
    rows = [  # (base, gestures, voice, status)
        (3, good(0), 0, 0),
        (4, good(1), 1, 1),                                    # a base of 1 frame
        (2, good(2), 0, 0),
        (5, good(3), 0, 1),                                    # ... of none
        (6, good(4), 1, 1),                                    # ... of more than max_frames
        (7, good(5), 0, 1),                                    # base id behind the table
        (-1, good(6), 0, 1),                                   # ... and in front of it
        (3, good(7), 1, 0),
        (3, good(8), 2, 1),                                    # voice id outside the plan's voices
        (3, good(9), -1, 1),
        (1, [(R3, ADD) + point(3)] * 65, 0, 2),
        (2, [(R3, ADD) + point(3)] * 64, 1, 0),
        (3, good(10)[:2] + [(16, ADD) + point(3)], 0, 3),
        (3, [(R3, 2) + point(3)] + good(11)[:3], 1, 3),
        (3, good(12)[:1] + [(R3, MULTIPLY) + point(3, np.nan)], 0, 3),
        (3, [(R3, ADD, [5, 4], np.float32([1, 2])), (VELUM, ADD) + point(9, np.inf)], 0, 3),   # 3 before 4
        (0, good(13), 0, 0),
        (3, [(R3, ADD) + point(-1)], 1, 4),
        (3, good(14)[:2] + [(R3, ADD, [4, 9, 9], np.float32([1, 2, 3]))], 0, 4),
        (3, [(R3, ADD, list(range(100, 300)) + [299], np.arange(201, dtype=np.float32))], 0, 4),  # (more points than lanes)
        (3, good(15), 1, 0),
    ]
    batch = Batch(bases, [r[1] for r in rows], [r[2] for r in rows], base_ids=[r[0] for r in rows])
    status, _ = check_apply(plan, batch, what="refused")
    assert status.tolist() == [r[3] for r in rows]


def test_offsets_that_decrease_are_refused(plan):
    """What the host entry is never given: the last utterance's gesture range, and its last gesture's point range, end in
    front of their start (the last, so that no other utterance's range changes)."""
    gestures, voices = drawn(5, 21)
    gestures[4] = gestures[4][:1] + pool("male")[:2]

    def fewer_gestures(t):
        t["utt_gestures"][-1] = t["utt_gestures"][-2] - 1

    def fewer_points(t):
        t["gesture_offsets"][-1] = t["gesture_offsets"][-2] - 1

    for doctor in (fewer_gestures, fewer_points):
        batch = Batch(shared_bases(), gestures, voices, base_ids=[3, 2, 3, 1, 3], doctor=doctor, status_of={4: 2})
        status, _ = check_apply(plan, batch, what=doctor.__name__)
        assert status.tolist() == [0, 0, 0, 0, 2]


def test_batch_of_none(plan):
    lib = plan._lib
    assert lib.gvtm_apply_modifications_device(plan._h, None, None, 0, None, None, None, None, None, None, None, 0, 0, None, None, None, None) == 0
    assert lib.gvtm_synthesize_modified_device(plan._h, None, None, 0, None, None, None, None, None, None, None, 0, 0, None, 0, None, None, None, None, None) == 0


def spoken(batch_size, seed):
    """Utterances of 17 frames that can be spoken -- tracks of the parity tests -- under three gentle gestures: ADD on r3,
    MULTIPLY on the frication volume, and a second ADD on r3 that starts later."""
    bases = list(tracks.random_tracks(batch_size, 17, seed0=seed, consonant_heavy=True))
    gestures = []
    for b in range(batch_size):
        cs = cases.PLANS[VOICE_KEYS[b % 2]].cs
        gestures.append([(R3, ADD, [b, 3 * cs + 7], np.float32([0.1, 0.25])), (FRIC_VOL, MULTIPLY, [2 * cs, 9 * cs + 1], np.float32([0.5, 1.5])),
                         (R3, ADD, [8 * cs + b, 12 * cs], np.float32([-0.2, 0.05]))][: 3 - b % 3 // 2])
    return bases, gestures


def test_one_call_equals_the_separate_calls(plan):
    """gvtm_synthesize_modified_device against gvtm_apply_modifications_device followed by gvtm_synthesize_voices_device:
    samples, counts, peaks, frame counts and statuses, as bytes."""
    n = 7
    bases, gestures = spoken(n, 700)
    gestures[2] = gestures[2] + [(R3, ADD, [4, 4], np.float32([1, 2]))]  # refused: 4
    voices = [b % 2 for b in range(n)]
    batch = Batch(bases, gestures, voices, max_frames=17)
    stride = plan.voices_output_capacity(17)

    def fresh():
        return dict(audio=filled((n, stride), 0.25, np.float32), frames=filled(n, 99, np.int32), counts=filled(n, 99, np.int64),
                    maxabs=filled(n, 5.0, np.float32), status=filled(n, -9, np.int32))

    two, one = fresh(), fresh()
    d_params = filled((n, 17, 16), 7.0, np.float32)
    plan.apply_modifications_device(*batch.inputs(), d_params, two["frames"], two["status"], current_stream())
    plan.synthesize_voices_device(d_params, batch.d_voices, n, 17, two["audio"], stride, two["frames"], two["counts"], two["maxabs"], current_stream())
    plan.synthesize_modified_device(*batch.inputs(), one["audio"], stride, one["frames"], one["counts"], one["maxabs"], one["status"], current_stream())
    two, one = dict(zip(two, to_host(*two.values()))), dict(zip(one, to_host(*one.values())))
    assert two["status"].tolist() == [0, 0, 4, 0, 0, 0, 0] and two["frames"].tolist() == [17, 17, 0, 17, 17, 17, 17]
    assert (two["counts"][two["status"] == 0] > 0).all() and (two["maxabs"][two["status"] == 0] > 0).all()
    for key in two:
        assert one[key].tobytes() == two[key].tobytes(), key
    # the plan's own frame counts serve when the caller gives none
    again = fresh()
    plan.synthesize_modified_device(*batch.inputs(), again["audio"], stride, None, again["counts"], again["maxabs"], None, current_stream())
    again = dict(zip(again, to_host(*again.values())))
    assert again["audio"].tobytes() == two["audio"].tobytes() and again["counts"].tobytes() == two["counts"].tobytes()
    assert (again["frames"] == 99).all() and (again["status"] == -9).all()


def test_end_to_end_against_the_oracle(plan):
    """Three utterances of 17 frames: the host rule's frames through the oracle's float class, the device's audio
    bit-identical."""
    bases, gestures = spoken(3, 800)
    voices = [0, 1, 0]
    batch = Batch(bases, gestures, voices, max_frames=17)
    stride = plan.voices_output_capacity(17)
    d_audio, d_counts, d_maxabs, d_status = filled((3, stride), 0.0, np.float32), filled(3, 0, np.int64), filled(3, 5.0, np.float32), filled(3, -9, np.int32)
    plan.synthesize_modified_device(*batch.inputs(), d_audio, stride, None, d_counts, d_maxabs, d_status, current_stream())
    audio, counts, maxabs, status = to_host(d_audio, d_counts, d_maxabs, d_status)
    assert status.tolist() == [0, 0, 0]
    refs = []
    for b in range(3):
        frames, st = capi.modification_apply_host(plan, bases[b], gestures[b], voice=voices[b])
        assert st == 0 and frames.tobytes() != bases[b].tobytes()
        refs.append(oracle.synthesize_batch(oracle_config(VOICE_KEYS[voices[b]], 44100.0, 1, 0, capi.PRECISION_F32), frames[None])[0])
    check_batch(audio, counts, maxabs, refs, True)


@pytest.mark.parametrize("key", ["male", "male5f", "male5"])
def test_other_plans_one_voice_and_null_ids(key):
    """A one-voice plan of the models 0 to 4, a gvtm_plan_create_model5_float plan and a double model 5 plan (N = 1208),
    two utterances each, null voice ids: frames-level parity, and the one-call entry runs the single-voice launch."""
    plan = cases.make_plan(key, 0)
    assert plan.modification_filter_length() == cases.filter_length(cases.PLANS[key].rate)
    names = [key + "__wide", key + "__hold"]
    inputs = [cases.case(n) for n in names]
    batch = Batch([base for _, base, _ in inputs], [gs for _, _, gs in inputs], None)
    status, frames = check_apply(plan, batch, n_voices=1, what=key)
    assert status.tolist() == [0, 0]
    fixture = dict(np.load(oracle.GOLDEN_DIR + "/modification_golden.npz", allow_pickle=False))
    for b, n in enumerate(names):
        assert cases.check_frames(fixture, n, frames[b]) is None
    # one call against two, on frames that can be spoken
    bases, gestures = spoken(2, 900)
    talk = Batch(bases, gestures, None, max_frames=17)
    stride = plan.output_capacity(17)
    outs = []
    for one_call in (False, True):
        o = dict(audio=filled((2, stride), 0.25, np.float32), frames=filled(2, 99, np.int32), counts=filled(2, 99, np.int64), maxabs=filled(2, 5.0, np.float32))
        if one_call:
            plan.synthesize_modified_device(*talk.inputs(), o["audio"], stride, o["frames"], o["counts"], o["maxabs"], None, current_stream())
        else:
            d_params = filled((2, 17, 16), 7.0, np.float32)
            plan.apply_modifications_device(*talk.inputs(), d_params, o["frames"], None, current_stream())
            plan.synthesize_device(d_params, 2, 17, o["audio"], stride, o["frames"], o["counts"], o["maxabs"], current_stream())
        outs.append(dict(zip(o, to_host(*o.values()))))
    assert outs[0]["frames"].tolist() == [17, 17] and (outs[0]["counts"] > 0).all()
    for k in outs[0]:
        assert outs[0][k].tobytes() == outs[1][k].tobytes(), (key, k)
