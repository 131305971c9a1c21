"""The case table of the posture-to-event-list rule (gvtm_rules_apply_host, gvtm_generate_events_device): posture sequences
for the compiled 0_male model (tests/golden/rules_model_0_male.npz) and for a small synthetic database whose text is
written here, so that its transitions can be what no shipped database dares.

tests/golden/make_rules_golden.py runs every case through the reference's Model and EventList
(tests/golden/ref_rules_table.cpp) and keeps, per case, the postures as the reference held them, its events, rule data,
onsets and exception in tests/golden/rules_golden.npz, with the compiled arrays of the synthetic database and the probes
that pin the compiler.  A text case goes through the reference's text parser and yields one golden entry per chunk of its
phonetic string, `<name>.0`, `<name>.1`, ...: the tests read postures from the golden file, never from the text.
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
MODEL_0_MALE = os.path.join(HERE, "golden", "rules_model_0_male.npz")
GOLDEN = os.path.join(HERE, "golden", "rules_golden.npz")

# ---------------------------------------------------------------------------------------------------------------------------
# the synthetic database

_PARAMS = ["p%d" % i for i in range(16)]
_RANGE = {5: (25.0, 70.0)}  # p5 clamps ordinary targets; every other parameter lies in [0, 100]


def _posture(symbol, categories, targets, symbols):
    cats = "".join('<category-ref name="%s"/>' % c for c in categories)
    par = "".join('<target name="%s" value="%s"/>' % (_PARAMS[i], repr(float(v))) for i, v in enumerate(targets))
    names = ("duration", "transition", "qssa", "qssb", "markedDuration", "markedTransition", "markedQssa", "markedQssb")
    sym = "".join('<target name="%s" value="%s"/>' % (n, repr(float(v))) for n, v in zip(names, symbols))
    return ('<posture symbol="%s"><posture-categories>%s</posture-categories><parameter-targets>%s</parameter-targets>'
            '<symbol-targets>%s</symbol-targets></posture>' % (symbol, cats, par, sym))


def _point(kind, value, time=None, free=None):
    when = 'time-expression="%s"' % time if time is not None else 'free-time="%s"' % free
    return '<point type="%s" value="%s" %s/>' % (kind, value, when)


def _ratio(points, slopes):
    return "<slope-ratio><points>%s</points><slopes>%s</slopes></slope-ratio>" % (
        "".join(points), "".join('<slope slope="%s"/>' % s for s in slopes))


def _transition(name, kind, items):
    return '<transition name="%s" type="%s"><point-or-slopes>%s</point-or-slopes></transition>' % (name, kind, "".join(items))


def _rule(expressions, profiles, specials, equations):
    e = "".join("<boolean-expression>%s</boolean-expression>" % x for x in expressions)
    p = "".join('<parameter-transition name="%s" transition="%s"/>' % (_PARAMS[i], t) for i, t in enumerate(profiles))
    s = "".join('<parameter-transition name="%s" transition="%s"/>' % (_PARAMS[i], t) for i, t in sorted(specials.items()))
    q = "".join('<symbol-equation name="%s" equation="%s"/>' % kv for kv in equations)
    return ("<rule><boolean-expressions>%s</boolean-expressions><parameter-profiles>%s</parameter-profiles><special-profiles>%s"
            "</special-profiles><expression-symbols>%s</expression-symbols></rule>" % (e, p, s, q))


def synthetic_xml():
    """The synthetic database's text: 11 postures, 4 rules."""
    a = [20.0 + i for i in range(16)]
    b = [60.0 - 2 * i for i in range(16)]
    a[4] = b[4] = 33.0                     # equal targets on p4, whose profile is then skipped: its special profile still runs
    sym = (100, 21.3, 33.7, 25.9, 100, 31.1, 47.3, 35.2)
    postures = [
        _posture("a", ["ca", "phone"], a, sym),
        _posture("b", ["cb", "phone"], b, (100, 18.9, 29.4, 22.2, 100, 27.7, 41.9, 30.6)),
        _posture("b2", ["cb", "phone"], a, sym),                         # a's targets in b's category: equal targets
        _posture("c", ["ca", "cb", "phone"], [96.5] * 16, sym),            # near every maximum
        _posture("l", ["ca", "phone"], [1.25] * 16, sym),                  # near every minimum
        _posture("n", ["never", "phone"], a, sym),                         # no rule starts with it
        _posture("z", ["phone"], a, sym),                                  # the rule of (int)duration 0
    ] + [_posture("t%d" % k, ["ct", "phone"], [10.0 * k + i if i != 10 else 50.0 for i in range(16)], (100, 20.5 + k, 30.25 + k, 24.5, 100, 30, 45, 33))
         for k in (1, 2, 3, 4)]
    equations = [
        ("zero", "0"), ("rdDi", "( qssa1 + transition1 + qssb2 ) / tempo1"), ("beatDi", "qssa1 * 0.5 / tempo1"),
        ("rd", "rd"), ("m1", "mark1"), ("m2", "mark2"), ("half", "rd * 0.5"), ("nearHalf", "rd * 0.5 + 0.45"),
        ("third", "rd / 3"), ("twoThirds", "rd * 2 / 3"), ("past", "rd + 2.5"), ("far", "rd + 100"), ("before", "- 5"),
        # (rd is evaluated first: it cannot read mark1 or mark2; mark2 may read mark1)
        ("mark1Tri", "( qssa1 + transition1 ) / tempo1"),
        ("rdTri", "( qssa1 + transition1 ) / tempo1 + ( qssa2 + transition2 ) / tempo2 + qssb3 / tempo3"),
        ("mark2Tetra", "mark1 + ( qssa2 + transition2 ) / tempo2"),
        ("rdTetra", "( qssa1 + transition1 ) / tempo1 + ( qssa2 + transition2 ) / tempo2 + ( qssa3 + transition3 ) / tempo3 + qssb4 / tempo4"),
        ("halfM1", "mark1 * 0.5"), ("midM1M2", "mark1 + ( mark2 - mark1 ) * 0.5"), ("midM2Rd", "mark2 + ( rd - mark2 ) * 0.5"),
        ("midM1Rd", "mark1 + ( rd - mark1 ) * +0.5"), ("tiny", "0.5"), ("tinyBeat", "0.25"),
    ]
    di, tri, tetra = "diphone", "triphone", "tetraphone"
    transitions = [
        _transition("lin", di, [_point(di, 0, "zero"), _point(di, 50, "half"), _point(di, 100, "rd")]),
        _transition("ratioFirst", di, [_ratio([_point(di, 0, "zero"), _point(di, 30, "third"), _point(di, 80, "half")], [1, 3]),
                                       _point(di, 90, "twoThirds"), _point(di, 100, "rd")]),
        _transition("ratioMid", di, [_point(di, 0, "zero"), _ratio([_point(di, 10, "third"), _point(di, 40, "half"), _point(di, 55, "nearHalf"),
                                                                     _point(di, 95, "twoThirds")], [2, 0.5, 1]), _point(di, 100, "rd")]),
        _transition("ratioLast", di, [_point(di, 0, "zero"), _point(di, 20, None, 7.5),
                                      _ratio([_point(di, 25, "third"), _point(di, 60, "twoThirds"), _point(di, 100, "rd")], [1, 2])]),
        _transition("phantom", di, [_point(di, 100, "rd")]),
        _transition("over", di, [_point(di, 0, "zero"), _point(di, 260, "third"), _point(di, -180, "twoThirds"), _point(di, 100, "rd")]),
        _transition("same", di, [_point(di, 0, "zero"), _point(di, 40, "half"), _point(di, 45, "nearHalf"), _point(di, 100, "rd")]),
        _transition("past", di, [_point(di, 0, "zero"), _point(di, 50, "before"), _point(di, 60, "half"), _point(di, 80, "past"), _point(di, 90, "far"),
                                 _point(di, 100, "rd")]),
        _transition("skipDi", di, [_point(di, 0, "zero"), _point(di, 70, "third"), _point(tetra, 30, "twoThirds"), _point(tetra, 100, "rd")]),
        _transition("linTri", tri, [_point(di, 0, "zero"), _point(di, 100, "m1"), _point(tri, 50, "midM1Rd"), _point(tri, 100, "rd")]),
        _transition("ratioTri", tri, [_point(di, 0, "zero"), _ratio([_point(di, 20, "halfM1"), _point(di, 100, "m1")], [1]),
                                      _ratio([_point(tri, 0, "m1"), _point(tri, 60, "midM1Rd"), _point(tri, 100, "rd")], [3, 1])]),
        _transition("linTetra", tetra, [_point(di, 0, "zero"), _point(di, 100, "m1"), _point(tri, 100, "m2"), _point(tetra, 50, "midM2Rd"),
                                        _point(tetra, 100, "rd")]),
        _transition("skipTetra", tetra, [_point(di, 0, "zero"), _point(di, 60, "halfM1"), _point(tetra, 40, "midM2Rd"), _point(tetra, 100, "rd")]),
    ]
    specials = [
        _transition("bump", di, [_point(di, 0, "zero"), _point(di, 12.5, "third"), _point(di, -4, "nearHalf"), _point(di, 0, "rd")]),
        _transition("late", di, [_point(di, 3, "half"), _point(di, 5, "past")]),
        _transition("bumpTri", tri, [_point(di, 0, "zero"), _point(tri, 8, "midM1Rd"), _point(tri, 0, "rd")]),
    ]
    di_profiles = ["lin", "ratioFirst", "ratioMid", "ratioLast", "phantom", "over", "same", "past", "skipDi"] + ["lin"] * 7
    rules = [
        _rule(["t1", "t2", "t3", "(t4 or ca)"], ["skipTetra"] + ["linTetra"] * 15, {2: "bumpTri"},
              [("rd", "rdTetra"), ("beat", "halfM1"), ("mark1", "mark1Tri"), ("mark2", "mark2Tetra")]),
        _rule(["(marked ca)", "cb", "(ca or t1)"], ["linTri", "ratioTri"] * 8, {1: "bumpTri", 4: "bumpTri"},
              [("rd", "rdTri"), ("beat", "halfM1"), ("mark1", "mark1Tri"), ("mark2", "rd")]),
        _rule(["z", "(not never)"], ["lin"] * 16, {}, [("rd", "tiny"), ("beat", "tinyBeat"), ("mark1", "tiny")]),
        _rule(["(((ca xor never) or (cb and (not never))) or ct)", "(not never)"], di_profiles, {4: "bump", 9: "late", 5: "bump"},
              [("rd", "rdDi"), ("beat", "beatDi"), ("mark1", "rdDi")]),
    ]
    return ('<?xml version="1.0" encoding="UTF-8"?><root><categories>%s</categories><parameters>%s</parameters><symbols>%s</symbols>'
            "<postures>%s</postures><equations><equation-group name=\"all\">%s</equation-group></equations>"
            "<transitions><transition-group name=\"all\">%s</transition-group></transitions>"
            "<special-transitions><transition-group name=\"all\">%s</transition-group></special-transitions><rules>%s</rules></root>" % (
                "".join('<category name="%s"/>' % c for c in ("phone", "ca", "cb", "ct", "never")),
                "".join('<parameter name="%s" minimum="%s" maximum="%s" default="0"/>' % ((n,) + _RANGE.get(i, (0.0, 100.0))) for i, n in enumerate(_PARAMS)),
                "".join('<symbol name="%s" minimum="0" maximum="500" default="100"/>' % n for n in (
                    "duration", "transition", "qssa", "qssb", "markedDuration", "markedTransition", "markedQssa", "markedQssb")),
                "".join(postures), "".join('<equation name="%s" formula="%s"/>' % e for e in equations), "".join(transitions), "".join(specials),
                "".join(rules)))


MODELS = ("0_male", "synthetic")

# ---------------------------------------------------------------------------------------------------------------------------
# the cases: name -> dict(model, cp, postures [(name, marked, tempo, rule_tempo)] or text, reference: run through the
# reference (False where it is undefined: the status is then the rule's own, 3))

CASES = {}


def _case(name, model, cp, postures=None, text=None, reference=True, repeat=0):
    assert name not in CASES
    CASES[name] = dict(model=model, cp=cp, postures=postures, text=text, reference=reference, repeat=repeat)


def _seq(names, marked=(), tempo=1.0, rule_tempo=1.0, tempos=None):
    return [(n, 1 if i in marked else 0, tempos[i] if tempos else tempo, rule_tempo) for i, n in enumerate(names)]


# 0_male: one diphone rule, one triphone rule (the database has no tetraphone rule), four postures
_case("m_two", "0_male", 4, _seq(["#", "a"]))
_case("m_three", "0_male", 4, _seq(["#", "m", "a"]))
_case("m_four", "0_male", 4, _seq(["#", "m", "a", "#"]))
for _cp in (1, 2, 3, 4):
    _case("m_cp%d" % _cp, "0_male", _cp, _seq(["#", "h", "e", "l", "uh", "uu", "#"], tempo=1.13))
_case("m_rule_tempo_half", "0_male", 4, _seq(["#", "m", "a", "s", "i", "#"], rule_tempo=0.5))
_case("m_rule_tempo_1p7", "0_male", 3, _seq(["#", "m", "a", "s", "i", "#"], rule_tempo=1.7))
for _m in range(8):  # marked postures at every position of the triphone rule
    _case("m_marked%d" % _m, "0_male", 4, _seq(["#", "m", "a", "#"], marked=[i for i in range(3) if _m >> i & 1]))
# tempos that shrink one interval or another below control period + 1, and one that shrinks none
_case("m_small_first", "0_male", 4, _seq(["#", "m", "a"], tempos=[40.0, 1.0, 1.0]))
_case("m_small_second", "0_male", 4, _seq(["#", "m", "a"], tempos=[1.0, 40.0, 40.0]))
_case("m_small_third", "0_male", 4, _seq(["#", "m", "a"], tempos=[1.0, 1.0, 40.0]))
_case("m_small_di", "0_male", 4, _seq(["a", "s"], tempo=60.0))
_case("m_fast_ok", "0_male", 1, _seq(["#", "a", "s", "#"], tempo=3.0))
_case("m_tempo_zero", "0_male", 4, _seq(["#", "a", "s"], tempos=[1.0, 0.0, 1.0]), reference=False)
_case("m_rule_tempo_zero", "0_male", 4, _seq(["#", "a"], rule_tempo=0.0), reference=False)
_case("m_one_posture", "0_male", 4, _seq(["a"]), reference=False)
# through the reference's text parser: "Hello world." (its chunks) and a sentence of about 60 postures
_case("hello", "0_male", 4, text="Hello world.")
_case("sentence", "0_male", 4, text="The quick brown fox jumps over the lazy dog near the river bank.", repeat=2000)

# the synthetic database
_case("s_di", "synthetic", 4, _seq(["a", "b"]))
for _cp in (1, 2, 3):
    _case("s_di_cp%d" % _cp, "synthetic", _cp, _seq(["a", "b", "c", "l", "a"], tempo=0.93))
_case("s_no_rule", "synthetic", 4, _seq(["a", "n", "b"]))
_case("s_no_rule_late", "synthetic", 4, _seq(["a", "b", "n", "a"]))
_case("s_clamp", "synthetic", 4, _seq(["c", "l", "c", "a"]))
_case("s_equal_di", "synthetic", 4, _seq(["a", "b2", "a"]))
_case("s_tri", "synthetic", 4, _seq(["a", "b", "a", "b"], marked=[0]))
_case("s_tri_cp3", "synthetic", 3, _seq(["l", "c", "t1", "t2"], marked=[0, 2], tempo=1.21))
_case("s_equal_tri", "synthetic", 4, _seq(["a", "b2", "a", "b"], marked=[0]))
_case("s_tetra", "synthetic", 4, _seq(["a", "t1", "t2", "t3", "t4", "b"]))
_case("s_tetra_cp2", "synthetic", 2, _seq(["t1", "t2", "t3", "a", "b"], tempo=0.77, rule_tempo=1.7))
_case("s_tetra_short", "synthetic", 4, _seq(["t1", "t2", "t3"]))          # three postures left: the tetraphone rule cannot match
_case("s_zero_duration", "synthetic", 4, _seq(["a", "z", "b"]))
_case("s_small_tri", "synthetic", 4, _seq(["a", "b", "a"], marked=[0], tempos=[30.0, 1.0, 1.0]))
_case("s_small_tri_last", "synthetic", 4, _seq(["a", "b", "a"], marked=[0], tempos=[1.0, 30.0, 30.0]))
_case("s_small_tetra", "synthetic", 4, _seq(["t1", "t2", "t3", "t4"], tempos=[1.0, 1.0, 40.0, 40.0]))
_case("s_small_tetra_mid", "synthetic", 4, _seq(["t1", "t2", "t3", "t4"], tempos=[1.0, 40.0, 1.0, 1.0]))
_case("s_window_one", "synthetic", 4, _seq(["a", "b", "a", "b"], tempo=14.0))  # rules of 5 to 7 ms: windows of one control period
_case("s_window_one_cp2", "synthetic", 2, _seq(["a", "b", "c", "l", "a", "b"], tempo=24.0))
_case("s_bad_posture", "synthetic", 4, [("a", 0, 1.0, 1.0), (99, 0, 1.0, 1.0)], reference=False)
_case("s_nan_tempo", "synthetic", 4, _seq(["a", "b"], tempos=[float("nan"), 1.0]), reference=False)

def chunk_names(golden):
    """Every golden entry's name, in the order of the cases."""
    return [str(n) for n in golden["names"]]


def entries_of(golden, model, cp):
    """The entries of one model under one control period: what one gvtm_generate_events_device call can hold."""
    return [n for n in chunk_names(golden) if MODELS[int(golden[n + "__model"])] == model and int(golden[n + "__cp"]) == cp]


def posture_records(golden, name):
    """The postures of a golden entry as (id, marked, tempo, rule_tempo) rows."""
    return np.asarray(golden[name + "__postures"], dtype=np.float64).reshape(-1, 4)


def model_arrays(golden, model):
    """The compiled arrays of a model: the committed 0_male fixture, or the synthetic database's out of the golden file."""
    if model == "0_male":
        return dict(np.load(MODEL_0_MALE))
    return {k[len("synthetic__"):]: golden[k] for k in golden.files if k.startswith("synthetic__")}


def expected_status(golden, name):
    """0, or what the reference's exception maps to; for a case the reference is not run on, the rule's own status."""
    return int(golden[name + "__status"])


# statuses of the cases the reference is undefined on (the rule refuses them on its own)
OWN_STATUS = {"m_tempo_zero": 3, "m_rule_tempo_zero": 3, "m_one_posture": 4, "s_bad_posture": 4, "s_nan_tempo": 3}
