"""Fixtures of the five reference model 5 voices (the variants of data/voice/english/5_male: tests/golden/voice5_*.txt).

Shared by tests/golden/make_voices5_golden.py (runs the REAL reference, oracle/_ref/ref_vtm, on the four voices besides
male), tests/test_oracle5_voices_vs_golden.py and tests/test_gpu_voices5.py.  Every case: VocalTractModel5<double,1> at a
250 Hz control rate and 48 kHz output (one overrun case: 44.1 kHz), one voice file, one track recipe
(golden_cases.track_for); "full" stores the output, "digest" a strided subset, "tail" that and the last OVERRUN_TAIL samples.
"""
import golden_cases
import oracle
import voice_files

NEW_VOICES = voice_files.VOICES[1:]
RATE, CRATE = 48000.0, 250.0

# Internal rate (331.4 + 0.6 * 35) * 30 * 100 / L Hz (VocalTractModel5.h:462-465) and control steps per 250 Hz frame
TRACT_CM = {"male": 17.5, "female": 15.0, "large_child": 12.5, "small_child": 10.0, "baby": 7.5}
STEPS_PER_FRAME = {"male": 242, "female": 282, "large_child": 338, "small_child": 423, "baby": 564}

# a frame count of each voice whose converter runs into the flush overrun (an extra lap of the 1024-sample ring after the
# last automatic dataEmpty(); vtm_design.hpp: src_flush_overrun), and its output rate: the shortest at 48 kHz, except for
# female, which overruns at no length up to 6000 frames at 48 kHz (at 44.1 kHz: 167, 658, 2131, ...)
OVERRUN_FRAMES = {"female": 167, "large_child": 295, "small_child": 975, "baby": 337}
OVERRUN_RATE = {"female": 44100.0, "large_child": RATE, "small_child": RATE, "baby": RATE}
# what an overrun case stores besides the digest and the strided subset: the last samples (the extra lap and before it)
OVERRUN_TAIL = golden_cases.OVERRUN_TAIL


def oracle_config(name, rate=RATE):
    return oracle.config5_from_dict(oracle.read_config_file(voice_files.voice_path(name, model5=True)), rate)


def C(name, voice, track, store="full", rate=RATE):
    return dict(name=name, voice=voice, track=track, store=store, rate=rate)


CASES = []
for _i, _v in enumerate(NEW_VOICES):
    CASES += [
        C("%s_hello" % _v, _v, ("hello",), store="digest"),
        C("%s_cons" % _v, _v, ("random", 120, 50 + _i, True)),
        C("%s_ovr_%df" % (_v, OVERRUN_FRAMES[_v]), _v, ("random", OVERRUN_FRAMES[_v], 60 + _i, True), store="tail",
          rate=OVERRUN_RATE[_v]),
    ]

DIGEST_STRIDE = golden_cases.DIGEST_STRIDE
track_for = golden_cases.track_for
