"""Fixtures of VocalTractModel5<float,1> (oracle/ref_driver.cpp's model "5f") on the four 5_male variants besides male
(tests/golden/voice5_{female,large_child,small_child,baby}.txt), and of both classes of model 5 at the limits of the
sample-rate converter.

Shared by tests/golden/make_voices5f_golden.py (runs the REAL reference, oracle/_ref/ref_vtm),
tests/test_oracle5f_voices_vs_golden.py (the oracles), tests/test_capi_model5_float_voices_cpu.py (design-only plans) and
tests/test_gpu_model5_float_voices.py (the device).

Voice cases (model "5f", 250 Hz control rate, 48 kHz unless stated), the recipes of golden5_voices_cases.py:
<voice>_hello_5f ("digest": SHA-256 and every DIGEST_STRIDE-th sample), <voice>_cons_5f (120 consonant-heavy frames,
"full") and <voice>_ovr_5f ("tail": digest and the last OVERRUN_TAIL samples) at the voice's flush-overrun length -- the
float converter overruns at the lengths the double one does: female 167 frames at 44.1 kHz, large_child 295, small_child
975, baby 337 (count(f) > count(f + 1); make_voices5f_golden.py asserts it).

Converter-limit cases, 12 frames, "full", in both classes (model "5f" and "5"):
  male at 8 200 Hz and baby at 19 200 Hz: down-sampling pad 96, the largest the plans accept (vtm_design.hpp: kMaxPad; the
    kernel's ring is sized for it); baby has 564 steps per frame;
  female at 211 440 Hz: output rate / internal rate exactly 3.0 in float (70 480 Hz x 3), the largest ratio the plans
    accept.  In double the internal rate (331.4 + 0.6 * 35) * 3000 / 15 comes out as 70 480 Hz exactly as well, the
    ratio is exactly 3.0 and gvtm_plan_create_model5 accepts it: the double case uses the same rate (the next double
    above 211 440 Hz is refused)."""
import functools
import json
import os

import numpy as np

import golden5_voices_cases
import golden_cases
import oracle
import voice_files

NEW_VOICES = golden5_voices_cases.NEW_VOICES
RATE, CRATE = golden5_voices_cases.RATE, golden5_voices_cases.CRATE
STEPS_PER_FRAME = golden5_voices_cases.STEPS_PER_FRAME
OVERRUN_FRAMES = golden5_voices_cases.OVERRUN_FRAMES
OVERRUN_RATE = golden5_voices_cases.OVERRUN_RATE
OVERRUN_TAIL = golden_cases.OVERRUN_TAIL
DIGEST_STRIDE = golden_cases.DIGEST_STRIDE
track_for = golden_cases.track_for
GOLDEN = os.path.join(oracle.GOLDEN_DIR, "voices5f_golden.npz")

MAX_PAD = 96  # the largest down-sampling pad a model 5 plan accepts
LIMIT_TRACK = ("random", 12, 78, True)
# (voice, output rate, what the rate sits on)
LIMITS = [("male", 8200.0, "pad96"), ("baby", 19200.0, "pad96"), ("female", 211440.0, "ratio3")]
DOUBLE_RATIO3_RATE = 211440.0  # the highest rate the double class takes for female: 3.0 x, too (module docstring)


def C(name, voice, track, store="full", rate=RATE, model="5f"):
    return dict(name=name, voice=voice, track=track, store=store, rate=rate, crate=CRATE, model=model,
                float_model=1 if model == "5f" else 0)


VOICE_CASES = []
for _i, _v in enumerate(NEW_VOICES):
    VOICE_CASES += [
        C("%s_hello_5f" % _v, _v, ("hello",), store="digest"),
        C("%s_cons_5f" % _v, _v, ("random", 120, 50 + _i, True)),
        C("%s_ovr_5f" % _v, _v, ("random", OVERRUN_FRAMES[_v], 60 + _i, True), store="tail", rate=OVERRUN_RATE[_v]),
    ]

LIMIT_CASES = []
for _v, _rate, _what in LIMITS:
    LIMIT_CASES += [
        C("%s_%s_5f" % (_v, _what), _v, LIMIT_TRACK, rate=_rate),
        C("%s_%s_5" % (_v, _what), _v, LIMIT_TRACK, rate=DOUBLE_RATIO3_RATE if _what == "ratio3" else _rate, model="5"),
    ]

CASES = VOICE_CASES + LIMIT_CASES
FLOAT_CASES = [c for c in CASES if c["float_model"]]
DOUBLE_CASES = [c for c in CASES if not c["float_model"]]


@functools.lru_cache(maxsize=None)
def golden5fv():
    """tests/golden/voices5f_golden.npz: the reference's samples (full, strided, tail) and the manifest, loaded once."""
    z = np.load(GOLDEN, allow_pickle=False)
    data = {k: z[k] for k in z.files}
    data["manifest"] = json.loads(bytes(data.pop("manifest_json")).decode())
    return data


def oracle_config(voice, rate=RATE, float_model=1):
    return oracle.config5_from_dict(oracle.read_config_file(voice_files.voice_path(voice, model5=True)), rate, float_model)


def stored(case, out):
    """[(what `out` has to equal, the array's key in the fixture)] of a case, as its store says."""
    name = case["name"]
    if case["store"] == "full":
        return [(out, name + "__out")]
    parts = [(out[::DIGEST_STRIDE], name + "__strided")]
    if case["store"] == "tail":
        parts.append((out[-OVERRUN_TAIL:], name + "__tail"))
    return parts
