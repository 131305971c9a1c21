"""The case table of rhythm and intonation-point placement (gvtm_prosody_rhythm_host, gvtm_prosody_points_host,
gvtm_apply_rhythm_device, gvtm_place_intonation_device, gvtm_synthesize_prosody_device): utterances of the compiled 0_male
model (tests/golden/rules_model_0_male.npz) as the calls that build them.

tests/golden/make_prosody_golden.py runs every case through the reference's EventList (tests/golden/ref_prosody_table.cpp):
a table case through its public builder calls, in the order PhoneticStringParser makes them, a text case through the text
parser, chunk by chunk (`<name>.0`, `<name>.1`, ...).  It keeps, per entry, in tests/golden/prosody_golden.npz: the postures
before and after applyRhythm(), the closed feet and tone groups, the parameter set and the two draws the reference took per
group and per foot, the rule data and onsets, the IntonationPoints and the merged list after applyIntonation() with macro
intonation on.  The tests read tables from the golden file, never from the calls below.  The cases the reference cannot
build or is not asked about carry their tables here (OWN).

A table case is a list of calls:
    ("p", name, marked, tempo, rule_tempo)   newPostureWithObject, setCurrentPostureTempo, setCurrentPostureRuleTempo
    ("foot",)                                newFoot: closes the open foot at the current posture
    ("mark",) / ("ftempo", value)            setCurrentFootMarked / setCurrentFootTempo, of the open foot
    ("group",)                               newToneGroup: closes the open group and the open foot
    ("type", t)                              setCurrentToneGroupType, of the open group (0..4; a group never typed is `none`)
The first foot opens at posture 0 and the first group at foot 0.  What is open at the end is not listed: postures behind
the last closed foot lie in no foot.
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "prosody_golden.npz")

CASES = {}


def _case(name, cp=4, ops=None, text=None, seed=None, fixed=None, intonation_factor=1.0, global_tempo=1.0):
    """seed None: randomIntonation() false; fixed: the five fixed intonation parameters, or None (the tone-group files')."""
    assert name not in CASES
    CASES[name] = dict(cp=cp, ops=ops, text=text, seed=seed, fixed=fixed, intonation_factor=intonation_factor, global_tempo=global_tempo)


def _p(names, marked=False, tempo=1.0):
    return [("p", n, 1 if marked else 0, tempo, 1.0) for n in names]


def _foot(names, marked=False, ftempo=None, close="foot"):
    """One foot's postures, its marks, and the call that closes it."""
    ops = _p(names, marked)
    if marked:
        ops.append(("mark",))
    if ftempo is not None:
        ops.append(("ftempo", ftempo))
    return ops + [(close,)]


TAIL = _p(["#", "^"])  # what the parser leaves behind the last foot: in no foot

HEAD = _foot(["^", "#"])  # (newFoot closes nothing before the second posture, newToneGroup nothing before the second foot)

# one group with one tonic foot; a second group of one foot of one posture: its feet start and end at one onset (deltaTime 0)
_case("one_tonic", ops=[("type", 0)] + HEAD + _foot(["h", "e", "l", "uh", "uu"], marked=True, close="group") + TAIL)
_case("delta_zero", ops=[("type", 0)] + HEAD + _foot(["m", "a"], marked=True, close="group") + [("type", 0)] + _foot(["s"], close="group") + _p(["i", "t"]) + TAIL)
# feet without a vocoid (the first, and one between two that have one)
_case("no_vocoid", ops=[("type", 0)] + HEAD + _foot(["m", "a"]) + _foot(["s", "t"]) + _foot(["m", "a", "s"], marked=True, close="group") + TAIL)
# two feet of one posture each inside the triphone rule of "# m a": equal beats, so the second point is pushed by 2 * cp;
# with the files' time_offset of -40 ms the early points' beat + offset is also negative before the push
_case("one_rule", ops=[("type", 0)] + HEAD + _foot(["m"]) + _foot(["a"]) + _foot(["s", "i"], marked=True, close="group") + TAIL)
for _cp in (1, 2, 3):
    _case("one_rule_cp%d" % _cp, cp=_cp, ops=CASES["one_rule"]["ops"])
# a point whose beat + offset is negative.  The first point's cannot be (its offset is 0 and no list the rule accepts has a
# negative beat); the second's is where speech is fast enough for the first rule's beat (34 ms) to lie below the 40 ms of
# time_offset: both feet hang on the triphone rule of "# m a".  Its time is then clamped to 0 BEFORE the push, so what the
# point stores, beat + offset + (minTime - 0) = 36 ms, is not minTime (42 ms)
_case("negative_time", ops=[("type", 0)] + _p(["#", "m"], tempo=3.0) + [("foot",)] + _p(["a"], tempo=3.0) + [("foot",)] +
      _p(["s", "i"], marked=True, tempo=3.0) + [("mark",), ("group",)] + TAIL)
# a continuation group, a group never typed, and an exclamation with a question behind it
_case("continuation", ops=[("type", 3)] + _foot(["#", "m", "a"]) + _foot(["s", "i", "t"], marked=True, close="group") + TAIL)
_case("type_none", ops=_foot(["#", "m", "a"]) + _foot(["s", "i", "t"], marked=True, close="group") + TAIL)
_case("two_groups", ops=[("type", 1)] + _foot(["#", "h", "e"]) + _foot(["l", "uh"], marked=True, close="group") + [("type", 2)] + _foot(["uu", "m"]) +
      _foot(["a", "s"], marked=True, close="group") + TAIL)
_case("three_groups", ops=[("type", 3)] + HEAD + _foot(["h", "e"], marked=True, close="group") + [("type", 4)] + _foot(["l", "uh"]) +
      _foot(["uu", "m"], marked=True, close="group") + [("type", 0)] + _foot(["a", "s"]) + _foot(["i", "t", "a"], marked=True, close="group") + TAIL)
# /f foot tempi that hit both clamps (min_tempo 0.2, max_tempo 2.0), one that hits neither; a closed foot behind the last group
_case("clamps", ops=[("type", 0)] + _foot(["#", "m", "a"], ftempo=-3.0) + _foot(["s", "i"], ftempo=5.0) + _foot(["t", "a", "m"], marked=True, ftempo=0.75, close="group") +
      _foot(["i", "s"], ftempo=1.5) + TAIL)
_case("outside_feet", ops=[("type", 0)] + HEAD + _foot(["m", "a"], marked=True, close="group") + _p(["s", "i", "t", "#", "^"], tempo=1.25))
_case("ends_closed", ops=[("type", 0)] + _foot(["#", "m", "a"]) + _foot(["s", "i", "#"], marked=True, close="group"))
_case("global_tempo", global_tempo=0.7, ops=CASES["two_groups"]["ops"])
_case("factor_half", intonation_factor=0.5, ops=CASES["two_groups"]["ops"])
_case("fixed", fixed=(-1.5, 2.25, 3.0, -6.5, 2.0), ops=CASES["two_groups"]["ops"])
for _seed in (1, 20240229, 4294967295):
    _case("random_%d" % _seed, seed=_seed, ops=CASES["three_groups"]["ops"])
_case("random_fixed", seed=7, fixed=(-1.5, 2.25, 3.0, -6.5, 2.0), ops=CASES["two_groups"]["ops"])
# exactly 64 points: 31 tonic feet (62 points), one pretonic foot and the closing point
_VOWELS = ["a", "i", "e", "uh", "uu"]
_case("points_64", ops=[("type", 0)] + _foot(["#", "a"]) + sum((_foot(["s", _VOWELS[k % 5]], marked=True) for k in range(30)), []) +
      _foot(["m", "a"], marked=True, close="group") + TAIL)
_case("hello", text="Hello world.")
_case("sentence", text="The quick brown fox jumps over the lazy dog near the river bank.")
_case("sentence_random", text="The quick brown fox jumps over the lazy dog near the river bank.", seed=99)

# ---------------------------------------------------------------------------------------------------------------------------
# Refusals: tables of our own over the postures of a golden entry (the reference could not have built them, or is not
# asked).  name -> (entry whose postures, rule data and onsets are used, feet rows (start, end, marked, tempo), group rows
# (start_foot, end_foot, type), the status of gvtm_prosody_points_host, the status of gvtm_prosody_rhythm_host)
_STATEMENT = (2.0, -2.0, 4.0, -8.0, 4.0)
OWN = {
    # 65 points: 32 tonic feet and the closing point, over points_64's 66 postures
    "points_65": ("points_64", [(2 * k, 2 * k + 1, 1, 1.0) for k in range(32)], [(0, 31, 0)], 3, 0),
    "foot_outside": ("one_tonic", [(0, 1, 0, 1.0), (2, 99, 1, 1.0)], [(0, 1, 0)], 1, 1),
    "foot_negative": ("one_tonic", [(-1, 1, 0, 1.0)], [(0, 0, 0)], 1, 1),
    "foot_reversed": ("one_tonic", [(0, 1, 0, 1.0), (4, 3, 1, 1.0)], [(0, 1, 0)], 1, 1),
    "feet_overlap": ("one_tonic", [(0, 2, 0, 1.0), (2, 4, 1, 1.0)], [(0, 1, 0)], 1, 1),
    "feet_decrease": ("one_tonic", [(3, 4, 0, 1.0), (0, 1, 1, 1.0)], [(0, 1, 0)], 1, 1),
    "group_outside": ("one_tonic", [(0, 1, 0, 1.0), (2, 4, 1, 1.0)], [(0, 2, 0)], 1, 0),
    "group_reversed": ("one_tonic", [(0, 1, 0, 1.0), (2, 4, 1, 1.0)], [(1, 0, 0)], 1, 0),
    "groups_overlap": ("one_tonic", [(0, 1, 0, 1.0), (2, 4, 1, 1.0)], [(0, 1, 0), (1, 1, 0)], 1, 0),
    "group_type": ("one_tonic", [(0, 1, 0, 1.0), (2, 4, 1, 1.0)], [(0, 1, 6)], 1, 0),
    "tempo_nan": ("one_tonic", [(0, 1, 0, float("nan")), (2, 4, 1, 1.0)], [(0, 1, 0)], 0, 4),
    "no_group": ("one_tonic", [(0, 1, 0, 1.0), (2, 4, 1, 1.0)], [], 0, 0),
}


def own_tables(name):
    """-> (entry, feet rows [n][4], group rows [n][8] with the statement file's first parameter set, points status, rhythm status)"""
    entry, feet, groups, status, rhythm_status = OWN[name]
    return (entry, np.asarray(feet, dtype=np.float64).reshape(-1, 4), np.asarray([g + _STATEMENT for g in groups], dtype=np.float64).reshape(-1, 8), status,
            rhythm_status)


def entry_names(golden):
    """Every golden entry's name, in the order of the cases."""
    return [str(n) for n in golden["names"]]


def entries_of(golden, cp):
    """The entries under one control period: what one device call can hold."""
    return [n for n in entry_names(golden) if int(golden[n + "__cp"]) == cp]
