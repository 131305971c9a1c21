"""Parameter targets under a mix of voices in one launch (gvtm_synthesize_targets_voices_device; vtm_synth_kernel with the
voices and the targets flag together, csrc/vtm_kernels_targets_voices.hip, behind the check and the grouping kernel).

The bar is the project's rule for voices: in every precision voice v's utterances come out bit for bit -- samples, counts,
peaks -- as gvtm_synthesize_targets_device synthesizes them on a one-voice plan of configs[v], built with the same forced
rows and fed voice v's utterances in their batch order.  That entry is pinned to the oracle (test_gpu_targets.py); one test
here holds the new route to the oracle on its own.  Every audio buffer starts as a guard pattern, and everything behind a
row's count must still be the pattern.

The lists are spoken (targets_cases.spoken_lists); the step counts sit at the edges of a block of four steps, of the chunk
and of each voice's own filter length, which differs from voice to voice.

Rows: a launch has one shape for all its voices, and a voice that down-samples (the baby voice at 44.1 kHz; at SectionDelay 2
every voice but the male one) holds it to two rows, as test_gpu_voice_keys.py has it.  So the mixes with such a voice run
their forced four rows as two, and a mix of up-sampling voices beside each runs the four-row kernels."""
import numpy as np
import pytest

import gama_tts_amd as g
from gama_tts_amd import capi
import oracle
import targets_cases as cases
import voices_matrix_cases
from device_io import filled, to_device, to_host
from parity_rules import check_batch
from targets_io import GUARD, guard_behind_counts, run_targets
from voice_cases import configs, configs5, oracle_config

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT, UNSUPPORTED = 1, 4
BAD_VOICE = 5
CRATE = 250.0


def singles(cfgs, utterances, step_counts, voice_ids, rows, max_steps):
    """Voice v's utterances, in their batch order, through gvtm_synthesize_targets_device on a one-voice plan of cfgs[v] (the
    diagnostics library's forced to `rows`; 0: the product's) -> {b: (samples up to the count, count, maxabs)}."""
    out = {}
    for v, cfg in enumerate(cfgs):
        mine = [b for b, w in enumerate(voice_ids) if w == v]
        if not mine:
            continue
        plan = g.Plan(cfg, CRATE, 0, diagnostics=bool(rows), rows=rows)
        audio, counts, maxabs, statuses = run_targets(plan, [utterances[b] for b in mine], [step_counts[b] for b in mine], max_steps=max_steps)
        assert not statuses.any() and guard_behind_counts(audio, counts)
        for i, b in enumerate(mine):
            assert counts[i] == plan.targets_output_count(step_counts[b])
            out[b] = (audio[i, : counts[i]].copy(), int(counts[i]), maxabs[i])
        plan.close()
    return out


def assert_as_singles(got, refs, what):
    audio, counts, maxabs = got[:3]
    for b, (samples, count, peak) in refs.items():
        assert counts[b] == count, (what, b)
        assert audio[b, :count].tobytes() == samples.tobytes(), (what, b)
        assert maxabs[b].tobytes() == peak.tobytes(), (what, b)


def config_of(name, precision, delay):
    """A voice of voice_files.py, or "half50": the male voice at the tract length of targets_cases.HALF50_OVERRIDES, whose
    internal rate and window are a little longer than the male voice's and which up-samples as it does."""
    if name != "half50":
        return configs(44100.0, delay, precision, names=[name])[0]
    d = g.read_config_file(oracle.VOICE_MALE)
    d.update({k: str(v) for k, v in cases.HALF50_OVERRIDES.items()})
    return g.config_from_dict(d, 44100.0, delay, precision, 0)


def mixed_plan(names, precision, delay, rows):
    """-> (the configurations, the plan of those voices with `rows` forced (0: the product library), the rows a launch of up
    to 16 utterances has).  Four forced rows launch as two where a voice of the plan down-samples: its rows carry the
    reference's ring of 1024 samples, and four of those do not fit the LDS (as in test_gpu_voice_keys.py)."""
    cfgs = [config_of(n, precision, delay) for n in names]
    plan = g.VoicesPlan(cfgs, CRATE, 0, diagnostics=bool(rows), rows=rows)
    launched = voices_matrix_cases.voices_launch_shape(plan, 16)[0] if rows else 0
    assert launched == rows or (rows == 4 and launched == 2), (rows, launched)
    return cfgs, plan, launched


def check_mix(cfgs, plan, rows, voice_ids, step_counts, wide=()):
    """The batch on the plan of several voices against the one-voice plans at `rows`; utterance b speaks the lists of seed b."""
    utterances = [cases.spoken_lists(s, b, wide=b in wide) for b, s in enumerate(step_counts)]
    got = run_targets(plan, utterances, step_counts, voice_ids)
    assert not got[3].any()
    for b, s in enumerate(step_counts):
        assert got[1][b] == plan.targets_voice_output_count(voice_ids[b], s), b
    assert guard_behind_counts(got[0], got[1])
    assert_as_singles(got, singles(cfgs, utterances, step_counts, voice_ids, rows, max(step_counts)), rows)
    return got


# ---- a. float, every row count ----

# (the baby voice's internal rate is above 44.1 kHz: its plan launches at most two rows; the second set of voices launches four)
@pytest.mark.parametrize("names,four", [(["male", "female", "baby", "large_child"], False), (["male", "female", "small_child", "large_child"], True)],
                         ids=["with-baby", "up-sampling"])
@pytest.mark.parametrize("rows", [1, 2, 4])
def test_float_in_every_row_count(rows, names, four):
    cfgs, plan, launched = mixed_plan(names, capi.PRECISION_F32, 1, rows)
    chunk = {1: 144, 2: 96, 4: 48}[launched]
    assert (launched == rows or not four) and int(plan._lib.gvtm_debug_chunk_length(plan._h, 16)) == chunk
    n = [plan.targets_filter_length(v) for v in range(4)]
    assert len(set(n[:3])) == 3  # three windows of three lengths

    def edges(v):
        return [0, 1, 5, chunk + 1, n[v] - 1, n[v] + 1, 2 * n[v] + chunk + 3]

    # the first two voices at every edge, interleaved and unsorted; the third with one utterance (rows of its workgroup stay
    # empty); the fourth with none
    voice_ids = [1, 0, 0, 1, 2, 1, 0, 1, 0, 0, 1, 1, 0, 1, 0]
    left = {0: edges(0)[::-1], 1: edges(1)}
    step_counts = [left[v].pop() if v < 2 else 2 * n[2] + chunk + 3 for v in voice_ids]
    assert not left[0] and not left[1] and max(step_counts) < 6500
    wide = (voice_ids.index(2), step_counts.index(n[0] + 1), step_counts.index(n[1] + 1))  # one utterance per voice
    check_mix(cfgs, plan, launched, voice_ids, step_counts, wide)


# ---- b. fp64 and mixed: the same bar ----

@pytest.mark.parametrize("precision", [capi.PRECISION_F64, capi.PRECISION_MIXED], ids=["f64", "mixed"])
@pytest.mark.parametrize("rows", [1, 4])
def test_double_classes_are_bit_identical_too(precision, rows):
    cfgs, plan, launched = mixed_plan(["male", "female"], precision, 1, rows)
    assert launched == rows  # (both voices up-sample)
    chunk = int(plan._lib.gvtm_debug_chunk_length(plan._h, 16))
    n = [plan.targets_filter_length(v) for v in range(2)]
    assert n[0] != n[1]
    check_mix(cfgs, plan, launched, [1, 0, 1, 0, 1], [n[1] + 1, chunk + 1, chunk - 1, n[0] + chunk, n[0] - 1])


# ---- c. float, SectionDelay 2 (windows of about 2 000 steps; running-remainder bounds) ----

# (at SectionDelay 2 every voice but the male one is above 44.1 kHz and launches two rows; the male voice with a slightly
# shorter tube keeps four, and with them the running-remainder bounds of that shape)
@pytest.mark.parametrize("other", ["small_child", "half50"])
def test_float_section_delay_2_four_rows(other):
    cfgs, plan, launched = mixed_plan(["male", other], capi.PRECISION_F32, 2, 4)
    assert launched == 4 or other == "small_child"
    chunk = int(plan._lib.gvtm_debug_chunk_length(plan._h, 16))
    n = [plan.targets_filter_length(v) for v in range(2)]
    assert chunk == {2: 96, 4: 48}[launched] and n[0] == 2003 and n[1] != n[0]
    step_counts = [n[1] + 1, n[0] - 1, 2 * n[0] + chunk + 3, chunk + 1]
    assert max(step_counts) < 6500
    check_mix(cfgs, plan, launched, [1, 0, 0, 1], step_counts)


# ---- d. float against the oracle directly ----

def test_float_against_the_oracle():
    names = ["male", "female", "baby"]
    cfgs, plan, _ = mixed_plan(names, capi.PRECISION_F32, 1, 0)
    n = plan.targets_filter_length(1)
    step_counts = [n + 145, 0, 5, n - 1]
    voice_ids = [1, 0, 2, 1]
    utterances = [cases.spoken_lists(s, b) for b, s in enumerate(step_counts)]
    audio, counts, maxabs, statuses = run_targets(plan, utterances, step_counts, voice_ids)
    assert not statuses.any()
    cfg = oracle_config("female", 44100.0, 1, 0, capi.PRECISION_F32)
    rate = plan.voice_info(1).internal_rate_hz
    assert oracle.derive(cfg, rate).control_steps == 1
    mine, refs = [0, 3], []
    for b in mine:
        frames, status = capi.targets_apply_host(plan, utterances[b], step_counts[b], voice=1)
        assert status == 0
        refs.append(oracle.synthesize(cfg, frames, control_rate=rate))
        assert refs[-1].size == plan.targets_voice_output_count(1, step_counts[b])
    check_batch(audio[mine], counts[mine], maxabs[mine], refs, True)
    assert guard_behind_counts(audio, counts)


# ---- e. one set of lists under three voices ----

def test_shared_lists_across_voices():
    cfgs, plan, _ = mixed_plan(["male", "female", "baby"], capi.PRECISION_F32, 1, 0)
    lists = cases.spoken_lists(700, 3)
    ids = [list(range(16))] * 3
    got = run_targets(plan, lists, [700, 700, 700], [2, 0, 1], ids=ids)
    assert not got[3].any() and guard_behind_counts(got[0], got[1])
    assert len({got[0][b, : got[1][b]].tobytes() for b in range(3)}) == 3  # three speakers
    for b, v in enumerate([2, 0, 1]):
        single = g.Plan(cfgs[v], CRATE, 0)
        ref = run_targets(single, lists, [700], ids=ids[:1])
        assert got[1][b] == ref[1][0] and got[2][b].tobytes() == ref[2][0].tobytes()
        assert got[0][b, : got[1][b]].tobytes() == ref[0][0, : ref[1][0]].tobytes(), v
        single.close()


# ---- f. statuses ----

def test_refused_utterances_between_good_ones():
    cfgs, plan, _ = mixed_plan(["male", "female", "baby"], capi.PRECISION_F32, 1, 0)
    good = lambda seed: cases.spoken_lists(400, seed)  # noqa: E731

    def with_list(seed, p, steps, values):
        lists = good(seed)
        lists[p] = (steps, np.asarray(values, dtype=np.float32))
        return lists

    utterances = [good(0), good(1), good(2), good(3), good(4), good(5), with_list(6, 4, [0, 9], [1.0, np.nan]), with_list(7, 2, [5, 5], [1.0, 2.0]),
                  with_list(8, 15, [0, 7], [1.0, np.inf]), good(9), good(10)]
    voice_ids = [0, -1, 1, 3, 1, 2, 1, 2, 3, 2, 1]
    step_counts = [400, 300, 77, 300, -1, 300, 300, 300, 300, 1, 250]
    want = [0, BAD_VOICE, 0, BAD_VOICE, 1, 2, 3, 4, BAD_VOICE, 0, 0]

    def doctor(offsets, steps, values):
        offsets[5 * 16 + 3] = offsets[5 * 16 + 4] + 1  # utterance 5's list 3 ends before it begins

    audio, counts, maxabs, statuses = run_targets(plan, utterances, step_counts, voice_ids, max_steps=400, doctor=doctor)
    assert statuses.tolist() == want
    assert guard_behind_counts(audio, counts)
    # a voice outside the plan: left out
    for b in (1, 3, 8):
        assert counts[b] == -1 and maxabs[b] == 0.0
    # statuses 1 to 4: an utterance of 0 steps of its voice, the one-voice plan's
    for b in (4, 5, 6, 7):
        v = voice_ids[b]
        single = g.Plan(cfgs[v], CRATE, 0)
        empty = run_targets(single, [good(0)], [0], max_steps=400)
        zero = plan.targets_voice_output_count(v, 0)
        assert counts[b] == zero == empty[1][0] and maxabs[b].tobytes() == empty[2][0].tobytes()
        assert audio[b, :zero].tobytes() == empty[0][0, :zero].tobytes(), b
        single.close()
    # the good utterances' bytes, counts and peaks are those of the same batch without the refused ones
    keep = [b for b in range(len(want)) if want[b] == 0]
    alone = run_targets(plan, [utterances[b] for b in keep], [step_counts[b] for b in keep], [voice_ids[b] for b in keep], max_steps=400)
    assert not alone[3].any()
    for i, b in enumerate(keep):
        assert counts[b] == alone[1][i] == plan.targets_voice_output_count(voice_ids[b], step_counts[b])
        assert maxabs[b].tobytes() == alone[2][i].tobytes()
        assert audio[b, : counts[b]].tobytes() == alone[0][i, : counts[b]].tobytes(), b
    # no status asked for: the same audio; neither counts nor peaks asked for: the same audio
    silent = run_targets(plan, utterances, step_counts, voice_ids, max_steps=400, doctor=doctor, status=False)
    assert silent[0].tobytes() == audio.tobytes() and (silent[3] == -9).all() and silent[1].tolist() == counts.tolist()
    bare = run_targets(plan, utterances, step_counts, voice_ids, max_steps=400, doctor=doctor, counts=False, peaks=False)
    assert bare[0].tobytes() == audio.tobytes() and bare[3].tolist() == want and (bare[1] == -7).all() and (bare[2] == 5.0).all()


# ---- g. a plan of one voice ----

@pytest.mark.parametrize("kind", ["plan", "voices-plan"])
def test_one_voice(kind):
    cfg, = configs(44100.0, 1, capi.PRECISION_F32, names=["female"])
    plan = g.Plan(cfg, CRATE, 0) if kind == "plan" else g.VoicesPlan([cfg], CRATE, 0)
    n = plan.targets_filter_length()
    step_counts = [n + 1, 0, 145, 2 * n + 147, 5]
    assert plan.targets_voices_output_capacity(max(step_counts)) == plan.targets_output_capacity(max(step_counts))
    utterances = [cases.spoken_lists(s, b) for b, s in enumerate(step_counts)]
    a = run_targets(plan, utterances, step_counts, [0] * 5)
    b = run_targets(plan, utterances, step_counts)
    assert not a[3].any() and not b[3].any() and guard_behind_counts(a[0], a[1])
    assert a[0].tobytes() == b[0].tobytes() and a[1].tolist() == b[1].tolist() and a[2].tobytes() == b[2].tobytes()
    assert a[1].tolist() == [plan.targets_output_count(s) for s in step_counts]


# ---- h. refusals on a device ----

def test_refusals_on_a_device():
    offsets, steps, values = capi.pack_targets(cases.spoken_lists(10, 0))
    d_offsets, d_steps, d_values, d_voices = to_device(offsets, steps, values, np.zeros(1, np.int32))

    def entry(plan, d_audio, stride, voices=d_voices):
        return plan._lib.gvtm_synthesize_targets_voices_device(plan._h, capi._ptr(d_offsets), 16, None, capi._ptr(d_steps), capi._ptr(d_values), None,
                                                               capi._ptr(voices), 1, 10, capi._ptr(d_audio), stride, None, None, None, None)

    plan5 = g.VoicesPlan(configs5(names=["male", "female"]), CRATE, 0)
    stride5 = plan5.targets_voices_output_capacity(10)
    assert entry(plan5, filled((1, stride5), 0.0, np.float32), stride5) == UNSUPPORTED
    plan = g.VoicesPlan(configs(44100.0, 1, capi.PRECISION_F32, names=["baby", "male"]), CRATE, 0)
    stride = plan.targets_voices_output_capacity(10)
    d_audio = filled((1, stride * 4), GUARD, np.uint8)
    assert entry(plan, d_audio, stride, voices=None) == INVALID_ARGUMENT and b"null voice ids" in plan._lib.gvtm_last_error()
    assert entry(plan, d_audio, stride - 1) == INVALID_ARGUMENT and b"audio_stride" in plan._lib.gvtm_last_error()
    audio, = to_host(d_audio)
    assert (audio == GUARD).all()
    # nothing to do
    assert plan._lib.gvtm_synthesize_targets_voices_device(plan._h, None, 0, None, None, None, None, None, 0, 0, None, 0, None, None, None, None) == 0
