"""The cases of tests/golden/targets5_voices_golden.npz: reference model 5 as the editor's interactive window runs it
(VocalTractModel5<T,1>(config, interactive = true), see targets5_cases.py) under the four voices that fixture lacks --
voice5_female, _large_child, _small_child and _baby at 48 kHz, whose tracts of 15 to 7.5 cm give internal rates from about
70 to 141 kHz and filters of about 3 500 to 7 050 samples -- fed the frames gvtm_targets_apply_host(plan, voice = v) makes of
spoken target lists on a plan of all five voices.  The male voice is held to targets5_golden.npz.

A case is (voice, step count S).  Per voice and class the step counts are one past the chunk of each of the class's shapes
under several voices (csrc/vtm_kernel_m5.inc: m5_targets_shape, the one-utterance shapes: float 60 and 52, double 56), one
past the voice's own filter length N_v, and 2 N_v + chunk + 5 with the class's longest chunk.  A case's lists are
targets_cases.spoken_lists over the voice's longest case, with a seed of its own; the pitch list has a point every 211 steps,
so f0 moves from step to step through every window."""
import gama_tts_amd as g
from gama_tts_amd import capi
import targets_cases
from targets5_cases import MODEL, POLL, RATE, sha256_of_frames  # noqa: F401  (the same driver, rate and hash)
from voice_files import VOICES, voice_path

NEW_VOICES = VOICES[1:]  # female, large_child, small_child, baby: voice ids 1 to 4 of the five-voice plan
# chunk of the shape a diagnostics plan of several voices forces with rows 1 / rows 2, by class (the double class has one)
CHUNKS = {True: (60, 52), False: (56,)}
MALE_N = 3021


def configs5(float_class, names=VOICES, rate=RATE):
    precision = capi.PRECISION_F32 if float_class else capi.PRECISION_F64
    return [g.config5_from_dict(g.read_config_file(voice_path(n, True)), rate, precision) for n in names]


def voices_plan(float_class, names=VOICES, device=capi.DEVICE_NONE, rows=0, crate=250.0):
    """The model 5 plan of `names` in a class (gvtm_plan_create_model5_voices / _float_voices); rows != 0: the diagnostics
    library's with that shape forced (1: index 0, 2: index 1)."""
    return g.VoicesPlan(configs5(float_class, names), crate, device, diagnostics=bool(rows), rows=rows, float_model5=float_class)


def single_plan(float_class, name, device=capi.DEVICE_NONE, rows=0, crate=250.0):
    """The one-voice plan of a voice's configuration (gvtm_plan_create_model5 / _float)."""
    return g.Plan(configs5(float_class, [name])[0], crate, device, diagnostics=bool(rows), rows=rows, float_model5=float_class)


def step_counts(float_class, n):
    """The step counts the fixture holds for a voice whose filter has n samples, ascending."""
    chunks = CHUNKS[float_class]
    return sorted({c + 1 for c in chunks} | {n + 1, 2 * n + max(chunks) + 5})


def edges(chunk, n):
    """Every step count an utterance under a voice can go wrong at (the GPU test's two full voices)."""
    return [0, 1, 3, 4, 5, chunk - 1, chunk, chunk + 1, n - 1, n, n + 1, 2 * n + chunk + 5]


def name(float_class, voice, n_steps):
    return "%s__%s__s%d" % (MODEL[float_class], voice, n_steps)


def lists_of(voice, n_steps, n):
    """The 16 lists of case (voice, S) of a voice whose filter has n samples: (steps, values) each."""
    return targets_cases.spoken_lists(2 * n + 70, 300 + 7 * VOICES.index(voice) + n_steps % 7)


def frames_of(plan, voice, n_steps):
    """gvtm_targets_apply_host's frames of case (voice, S) under voice VOICES.index(voice) of the five-voice plan."""
    v = VOICES.index(voice)
    frames, status = capi.targets_apply_host(plan, lists_of(voice, n_steps, plan.targets_filter_length(v)), n_steps, voice=v)
    assert status == 0
    return frames


def all_cases(plan, float_class):
    """[(voice name, S)] of a class, by the five-voice plan's filter lengths."""
    return [(voice, s) for voice in NEW_VOICES for s in step_counts(float_class, plan.targets_filter_length(VOICES.index(voice)))]
