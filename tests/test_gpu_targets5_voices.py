"""Model 5 parameter targets under a mix of voices in one launch (gvtm_synthesize_targets_model5_voices_device;
vtm5_synth_kernel with the voices and the targets flag together, csrc/vtm_kernels_m5tv.hip and csrc/vtm_kernels_m5ftv.hip,
behind the check and the grouping kernel).

The bar is the project's rule for voices: in both classes voice v's utterances come out bit for bit -- samples, counts,
peaks -- as gvtm_synthesize_targets_model5_device synthesizes them on a one-voice plan of configs[v] with the same forced
shape (float: chunk 60 and chunk 52; double: chunk 56), fed voice v's utterances in their batch order.  One test holds the
new route to the real reference on its own (tests/golden/targets5_voices_golden.npz for the four voices
targets5_golden.npz lacks, that file for the male voice): the float class by bytes, the double class to
parity_rules.check_batch.  Every audio buffer starts as a guard pattern, and everything behind a row's count must still be
the pattern: the whole row for a row that was left out.

The lists are spoken (targets_cases.spoken_lists); the step counts sit at the edges of a block of four steps, of the chunk
and of each voice's own filter length, which runs from 3021 (male) to about 7050 samples (baby).  A launch is one workgroup
per utterance; no utterance is longer than 2 N_v + chunk + 5 steps."""
import os

import numpy as np
import pytest

import gama_tts_amd as g
from gama_tts_amd import capi
import oracle
import targets5_cases as cases5
import targets5_voices_cases as cases
from device_io import filled, to_device, to_host
from parity_rules import check_batch
from targets_cases import spoken_lists
from targets_io import GUARD, at_own_index, guard_behind_counts, run_targets
from voice_cases import configs
from voice_files import VOICES

pytestmark = pytest.mark.gpu

OK, INVALID_ARGUMENT, UNSUPPORTED = 0, 1, 4
BAD_VOICE = 5
ENTRY = "gvtm_synthesize_targets_model5_voices_device"
# (class, forced rows of both kinds of plan, chunk): every shape the variant has
SHAPES = [(True, 1, 60), (True, 2, 52), (False, 1, 56)]
SHAPE_IDS = ["float-chunk60", "float-chunk52", "double-chunk56"]


@pytest.fixture(scope="module")
def fixtures():
    return (np.load(os.path.join(oracle.GOLDEN_DIR, "targets5_voices_golden.npz")), np.load(os.path.join(oracle.GOLDEN_DIR, "targets5_golden.npz")))


class Singles:
    """The one-voice plans of a class at a forced shape, made once per voice, and voice v's utterances of a batch through
    gvtm_synthesize_targets_model5_device on them."""

    def __init__(self, float_class, rows, names=VOICES):
        self.float_class, self.rows, self.names, self.plans = float_class, rows, names, {}

    def plan(self, v):
        if v not in self.plans:
            self.plans[v] = cases.single_plan(self.float_class, self.names[v], device=0, rows=self.rows)
        return self.plans[v]

    def of(self, utterances, step_counts, voice_ids, max_steps):
        """-> {b: (samples up to the count, count, maxabs)} of the utterances whose voice is in the plan"""
        out = {}
        for v in sorted(set(w for w in voice_ids if 0 <= w < len(self.names))):
            mine = [b for b, w in enumerate(voice_ids) if w == v]
            plan = self.plan(v)
            audio, counts, maxabs, statuses = run_targets(plan, [utterances[b] for b in mine], [step_counts[b] for b in mine], max_steps=max_steps)
            assert not statuses.any() and guard_behind_counts(audio, counts)
            for i, b in enumerate(mine):
                assert counts[i] == plan.targets_output_count(step_counts[b])
                out[b] = (audio[i, : counts[i]].copy(), int(counts[i]), maxabs[i])
        return out

    def close(self):
        for plan in self.plans.values():
            plan.close()


def assert_as_singles(got, refs, what):
    audio, counts, maxabs = got[:3]
    for b, (samples, count, peak) in refs.items():
        assert counts[b] == count, (what, b)
        assert audio[b, :count].tobytes() == samples.tobytes(), (what, b)
        assert maxabs[b].tobytes() == peak.tobytes(), (what, b)


def shuffled_ids(batch, seed):
    """The lists of `batch` utterances in another order, and the ids that find them: the lists are not where 16 b + p looks."""
    order = np.random.default_rng(seed).permutation(batch * 16)
    ids = np.empty(batch * 16, dtype=np.int32)
    ids[order] = np.arange(batch * 16, dtype=np.int32)
    return order, ids.reshape(batch, 16)


# ---- a. as the one-voice plans, in every shape; implicit lists and list ids ----

# (the two voices that take every edge, the voice with a single utterance; a fourth voice of the five has none)
@pytest.mark.parametrize("shape,full,one", list(zip(SHAPES, [(4, 1), (3, 2), (4, 0)], [2, 4, 1])), ids=SHAPE_IDS)
def test_as_the_one_voice_plans(shape, full, one):
    float_class, rows, chunk = shape
    plan = cases.voices_plan(float_class, device=0, rows=rows)
    singles = Singles(float_class, rows)
    n = [plan.targets_filter_length(v) for v in range(5)]
    assert len(set(n)) == 5 and n[0] == cases.MALE_N and chunk in cases.CHUNKS[float_class]
    edges = {v: cases.edges(chunk, n[v]) for v in full}
    # two launches, between them every edge of both voices: interleaved and unsorted, so that no utterance sits at its
    # workgroup's index (the groups are sorted by voice); the third voice's one utterance in the first
    for half in (0, 1):
        mine = {full[0]: edges[full[0]][half::2], full[1]: edges[full[1]][1 - half::2][::-1]}
        voice_ids = [full[i % 2] for i in range(12)]
        step_counts = [mine[v].pop() for v in voice_ids]
        if half == 0:
            at = next(i for i in range(13) if not at_own_index(voice_ids[:i] + [one] + voice_ids[i:]))
            voice_ids.insert(at, one)
            step_counts.insert(at, n[one] + 1)
        assert not at_own_index(voice_ids) and max(step_counts) <= 2 * max(n) + chunk + 5
        utterances = [spoken_lists(s, 40 * half + b) for b, s in enumerate(step_counts)]
        refs = singles.of(utterances, step_counts, voice_ids, max(step_counts))
        # d_list_ids == NULL: utterance b walks the lists 16 b + p, whichever workgroup it runs in
        got = run_targets(plan, utterances, step_counts, voice_ids)
        assert not got[3].any() and guard_behind_counts(got[0], got[1])
        for b, s in enumerate(step_counts):
            assert got[1][b] == plan.targets_voice_output_count(voice_ids[b], s), b
        assert_as_singles(got, refs, (chunk, half, "implicit"))
        # list ids: the same lists stored in another order
        order, ids = shuffled_ids(len(step_counts), half)
        flat = [l for u in utterances for l in u]
        with_ids = run_targets(plan, [flat[i] for i in order], step_counts, voice_ids, ids=ids)
        assert not with_ids[3].any() and guard_behind_counts(with_ids[0], with_ids[1])
        assert_as_singles(with_ids, refs, (chunk, half, "ids"))
    singles.close()


# ---- b. against the reference directly ----

@pytest.mark.parametrize("float_class,rows,chunk", [(True, 0, 60), (True, 2, 52), (False, 0, 56)], ids=["float", "float-chunk52", "double"])
def test_against_the_reference(fixtures, float_class, rows, chunk):
    new, male = fixtures
    plan = cases.voices_plan(float_class, device=0, rows=rows)
    n = [plan.targets_filter_length(v) for v in range(5)]
    longest = max(cases.CHUNKS[float_class])
    batch = []  # (voice id, S, lists, reference samples)
    for v in (1, 2, 3, 4):
        for s in (2 * n[v] + longest + 5, chunk + 1, n[v] + 1):
            batch.append((v, s, cases.lists_of(VOICES[v], s, n[v]), new[cases.name(float_class, VOICES[v], s)]))
    for s in (chunk + 1, cases.MALE_N + 1):
        batch.append((0, s, cases5.lists_of(s), male[cases5.name(float_class, s)]))
    batch = [batch[i] for i in np.random.default_rng(5).permutation(len(batch))]
    voice_ids, step_counts = [c[0] for c in batch], [c[1] for c in batch]
    audio, counts, maxabs, statuses = run_targets(plan, [c[2] for c in batch], step_counts, voice_ids)
    assert not statuses.any()
    check_batch(audio, counts, maxabs, [c[3] for c in batch], float_class)
    assert guard_behind_counts(audio, counts)


# ---- c. one set of lists under five voices ----

@pytest.mark.parametrize("float_class", [True, False], ids=["float", "double"])
def test_shared_lists_across_five_voices(float_class):
    plan = cases.voices_plan(float_class, device=0)
    singles = Singles(float_class, 0)
    lists = spoken_lists(700, 3)
    voice_ids = [2, 0, 4, 1, 3]
    ids = [list(range(16))] * 5
    got = run_targets(plan, lists, [700] * 5, voice_ids, ids=ids)
    assert not got[3].any() and guard_behind_counts(got[0], got[1])
    assert len({got[0][b, : got[1][b]].tobytes() for b in range(5)}) == 5  # five speakers
    for b, v in enumerate(voice_ids):
        ref = run_targets(singles.plan(v), lists, [700], ids=ids[:1])
        assert got[1][b] == ref[1][0] == plan.targets_voice_output_count(v, 700) and got[2][b].tobytes() == ref[2][0].tobytes()
        assert got[0][b, : got[1][b]].tobytes() == ref[0][0, : ref[1][0]].tobytes(), v
    singles.close()


# ---- d. statuses ----

@pytest.mark.parametrize("float_class", [True, False], ids=["float", "double"])
def test_refused_utterances_between_good_ones(float_class):
    plan = cases.voices_plan(float_class, device=0)
    singles = Singles(float_class, 0)
    good = lambda seed: spoken_lists(400, seed)  # noqa: E731

    def with_list(seed, p, steps, values):
        lists = good(seed)
        lists[p] = (steps, np.asarray(values, dtype=np.float32))
        return lists

    utterances = [good(0), good(1), good(2), good(3), good(4), good(5), with_list(6, 4, [0, 9], [1.0, np.nan]), with_list(7, 2, [5, 5], [1.0, 2.0]),
                  with_list(8, 15, [0, 7], [1.0, np.inf]), good(9), good(10)]
    voice_ids = [0, -1, 4, 5, 1, 2, 3, 4, 5, 2, 1]
    step_counts = [400, 300, 77, 300, -1, 300, 300, 300, 300, 1, 250]
    want = [0, BAD_VOICE, 0, BAD_VOICE, 1, 2, 3, 4, BAD_VOICE, 0, 0]

    def doctor(offsets, steps, values):
        offsets[5 * 16 + 3] = offsets[5 * 16 + 4] + 1  # utterance 5's list 3 ends before it begins

    audio, counts, maxabs, statuses = run_targets(plan, utterances, step_counts, voice_ids, max_steps=400, doctor=doctor)
    assert statuses.tolist() == want
    assert guard_behind_counts(audio, counts)
    # a voice outside the plan: left out, the whole row still the pattern (guard_behind_counts above)
    for b in (1, 3, 8):
        assert counts[b] == -1 and maxabs[b] == 0.0
    # statuses 1 to 4: an utterance of 0 steps of its voice, the one-voice plan's
    for b in (4, 5, 6, 7):
        v = voice_ids[b]
        empty = run_targets(singles.plan(v), [good(0)], [0], max_steps=400)
        zero = plan.targets_voice_output_count(v, 0)
        assert counts[b] == zero == empty[1][0] and maxabs[b].tobytes() == empty[2][0].tobytes()
        assert audio[b, :zero].tobytes() == empty[0][0, :zero].tobytes(), b
    # the good utterances' bytes, counts and peaks are those of the same batch without the refused ones
    keep = [b for b in range(len(want)) if want[b] == 0]
    alone = run_targets(plan, [utterances[b] for b in keep], [step_counts[b] for b in keep], [voice_ids[b] for b in keep], max_steps=400)
    assert not alone[3].any()
    for i, b in enumerate(keep):
        assert counts[b] == alone[1][i] == plan.targets_voice_output_count(voice_ids[b], step_counts[b])
        assert maxabs[b].tobytes() == alone[2][i].tobytes()
        assert audio[b, : counts[b]].tobytes() == alone[0][i, : counts[b]].tobytes(), b
    # d_status, d_out_counts and d_maxabs left out in turn: the same audio, the others' values, the fill untouched
    silent = run_targets(plan, utterances, step_counts, voice_ids, max_steps=400, doctor=doctor, status=False)
    assert silent[0].tobytes() == audio.tobytes() and (silent[3] == -9).all() and silent[1].tolist() == counts.tolist()
    assert silent[2].tobytes() == maxabs.tobytes()
    uncounted = run_targets(plan, utterances, step_counts, voice_ids, max_steps=400, doctor=doctor, counts=False)
    assert uncounted[0].tobytes() == audio.tobytes() and uncounted[3].tolist() == want and (uncounted[1] == -7).all()
    assert uncounted[2].tobytes() == maxabs.tobytes()
    peakless = run_targets(plan, utterances, step_counts, voice_ids, max_steps=400, doctor=doctor, peaks=False)
    assert peakless[0].tobytes() == audio.tobytes() and peakless[3].tolist() == want and (peakless[2] == 5.0).all()
    assert peakless[1].tolist() == counts.tolist()
    singles.close()


# ---- e. plans of one voice ----

@pytest.mark.parametrize("kind", ["model5-plan", "float-voices-plan-of-one"])
def test_one_voice(kind):
    float_class = kind != "model5-plan"
    single = cases.single_plan(float_class, "small_child", device=0)
    plan = single if kind == "model5-plan" else cases.voices_plan(True, names=["small_child"], device=0)
    n = plan.targets_filter_length()
    chunk = 60 if float_class else 56
    step_counts = [n + 1, 0, chunk + 1, 2 * n + chunk + 5, 5]
    assert plan.targets_voices_output_capacity(max(step_counts)) == single.targets_output_capacity(max(step_counts))
    utterances = [spoken_lists(s, b) for b, s in enumerate(step_counts)]
    a = run_targets(plan, utterances, step_counts, [0] * 5)
    b = run_targets(single, utterances, step_counts)
    assert not a[3].any() and not b[3].any() and guard_behind_counts(a[0], a[1])
    assert a[0].tobytes() == b[0].tobytes() and a[1].tolist() == b[1].tolist() and a[2].tobytes() == b[2].tobytes()
    assert a[1].tolist() == [single.targets_output_count(s) for s in step_counts]


# ---- f. refusals on a device ----

def test_refusals_on_a_device():
    offsets, steps, values = capi.pack_targets(spoken_lists(10, 0))
    d_offsets, d_steps, d_values, d_voices = to_device(offsets, steps, values, np.zeros(1, np.int32))

    def entry(plan, d_audio, stride, voices=d_voices):
        return getattr(plan._lib, ENTRY)(plan._h, capi._ptr(d_offsets), 16, None, capi._ptr(d_steps), capi._ptr(d_values), None,
                                         capi._ptr(voices), 1, 10, capi._ptr(d_audio), stride, None, None, None, None)

    def untouched(d_audio):
        audio, = to_host(d_audio)
        return bool((audio == GUARD).all())

    # the models 0 to 4 have an entry of their own; a one-voice float plan has no launch of several voices
    for plan, word in ((g.VoicesPlan(configs(44100.0, 1, capi.PRECISION_F32, names=["baby", "male"]), 250.0, 0), b"gvtm_synthesize_targets_voices_device"),
                       (cases.single_plan(True, "female", device=0), b"no launch of several voices")):
        stride = plan.targets_voices_output_capacity(10)
        d_audio = filled((1, stride * 4), GUARD, np.uint8)
        assert entry(plan, d_audio, stride) == UNSUPPORTED and word in plan._lib.gvtm_last_error()
        assert untouched(d_audio)
    plan = cases.voices_plan(False, names=["baby", "male"], device=0)
    stride = plan.targets_voices_output_capacity(10)
    d_audio = filled((1, stride * 4), GUARD, np.uint8)
    assert entry(plan, d_audio, stride, voices=None) == INVALID_ARGUMENT and b"null voice ids" in plan._lib.gvtm_last_error()
    assert entry(plan, d_audio, stride - 1) == INVALID_ARGUMENT and b"audio_stride" in plan._lib.gvtm_last_error()
    assert untouched(d_audio)
    # nothing to do
    assert getattr(plan._lib, ENTRY)(plan._h, None, 0, None, None, None, None, None, 0, 0, None, 0, None, None, None, None) == OK
