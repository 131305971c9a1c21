"""gama_tts_amd/control_model.py against the reference's own Model: the compiled match tables and equation programs on the
probes of tests/golden/rules_golden.npz (every rule position on every posture, unmarked and marked; every equation on 300
symbol vectors, bit for bit), the committed 0_male fixture against a fresh compile where the reference's database is at
hand, the two grammars on texts of our own, and what gvtm_rules_create refuses."""
import os

import numpy as np
import pytest

import rules_cases as cases
from gama_tts_amd import capi, control_model

REF_ARTIC = "/root/reference/data/voice/english/0_male/artic.xml"


@pytest.fixture(scope="module")
def golden():
    return np.load(cases.GOLDEN)


@pytest.mark.parametrize("model", cases.MODELS)
def test_match_table_is_the_references_boolean_result(golden, model):
    arrays = cases.model_arrays(golden, model)
    probe = golden[model + "__probe_match"]
    assert probe.shape == arrays["match"].shape and probe.any()
    assert np.array_equal(arrays["match"], probe)
    # beyond a rule's positions the table is empty
    for r, n in enumerate(arrays["rule_n_expr"]):
        assert not arrays["match"][r, n:].any()


@pytest.mark.parametrize("model", cases.MODELS)
def test_programs_give_the_references_float_results_bit_for_bit(golden, model):
    arrays = cases.model_arrays(golden, model)
    probe, vectors = golden[model + "__probe_equations"], golden["probe_vectors"]
    assert probe.shape == (arrays["equation_offsets"].shape[0] - 1, vectors.shape[0]) and vectors.shape[0] >= 300
    assert (vectors[:, 12:16] < 0).any() and (np.abs(vectors[:, 12:16]) < 0.01).any()  # tempoN small and negative are among them
    for e in range(probe.shape[0]):
        ours = np.array([control_model.evaluate_equation(arrays, e, v) for v in vectors], dtype=np.float32).view(np.uint32)
        nan = np.isnan(probe[e].view(np.float32))
        assert np.array_equal(np.isnan(ours.view(np.float32)), nan), e
        assert np.array_equal(ours[~nan], probe[e][~nan]), e


def test_synthetic_fixture_is_the_compile_of_its_text(golden):
    fresh = control_model.compile_model(cases.synthetic_xml())
    for k in control_model.ARRAYS:
        assert fresh[k].dtype == golden["synthetic__" + k].dtype and np.array_equal(fresh[k], golden["synthetic__" + k], equal_nan=fresh[k].dtype.kind == "f"), k


def test_committed_0_male_fixture_is_a_fresh_compile_of_the_references_database():
    if not os.path.exists(REF_ARTIC):
        pytest.skip("the reference's articulatory database is not on this machine")
    fresh, kept = control_model.compile_model(REF_ARTIC), np.load(cases.MODEL_0_MALE)
    for k in control_model.ARRAYS + ("posture_names", "equation_names", "transition_names"):
        assert fresh[k].dtype == kept[k].dtype and fresh[k].shape == kept[k].shape and (fresh[k] == kept[k]).all(), k


def test_parse_float32_rounds_once():
    # 0.1 + 2^-30 lies nearer to the float above 0.1f than to 0.1f only when read exactly; through a double it still does
    for text in ("0.333333", "2500", "1e-3", "5.5", "16777217", "0.1000000014901161193847656250001", "-4.25"):
        assert control_model.parse_float32(text) == np.float32(np.longdouble(text)), text
    assert control_model.parse_float32("16777217") == np.float32(16777216.0)  # a tie: to even
    assert control_model.parse_float32("16777219") == np.float32(16777220.0)


def test_formula_grammar():
    ops, consts = control_model.compile_formula("- ( rd - mark1 ) * +0.5 / 2 + tempo1")
    sym = np.zeros(21, dtype=np.float32)
    sym[[16, 18, 12]] = 100.0, 30.0, 1.5
    assert control_model.evaluate_program(ops, consts, sym) == np.float32(-(100.0 - 30.0) * 0.5 / 2 + 1.5)
    for bad in ("", "rd *", "( rd", "rd ) ", "rd*0.5", "1 2", "* 3"):
        with pytest.raises(control_model.ModelError):
            control_model.compile_formula(bad)


def test_boolean_grammar():
    ids, members = {"a": 0, "b": 1}, {"v": {0, 2}, "w": {1, 2}}
    def run(text):
        return list(control_model.compile_boolean(text, ids, members, 3))
    assert run("v") == [3, 0, 3] and run("a") == [3, 0, 0]
    assert run("(marked v)") == [2, 0, 2] and run("(not (marked v))") == [1, 3, 1]
    assert run("((v xor w) or b)") == [3, 3, 0] and run("(v and w)") == [0, 0, 3]
    for bad in ("", "(v)", "(v and)", "v w", "(v nor w)", "unknown", "(v or w"):
        with pytest.raises(control_model.ModelError):
            control_model.compile_boolean(bad, ids, members, 3)


def test_rules_create_refuses_what_the_reference_throws_at(golden):
    good = cases.model_arrays(golden, "synthetic")
    capi.Rules(good).close()
    ratio = int(np.flatnonzero(good["items"][:, 0] == control_model.ITEM_SLOPE_RATIO)[0])

    def refused(change, says):
        model = {k: np.array(v) for k, v in good.items()}
        change(model)
        with pytest.raises(capi.GvtmError) as e:
            capi.Rules(model)
        assert e.value.status == 1 and says in str(e.value), str(e.value)

    def fewer_slopes(m):
        m["items"][ratio, 4] -= 1

    def empty_ratio(m):
        m["items"][ratio, 2:5:2] = 0

    def no_profile(m):
        m["rule_param_transition"][1, 3] = -1

    def special_with_ratio(m):
        m["rule_special_transition"][0, 0] = int(np.searchsorted(m["transition_offsets"], ratio, side="right")) - 1

    def pops_empty(m):
        m["program_op"][m["equation_offsets"][1]] = control_model.OP_ADD

    def bad_symbol(m):
        m["program_op"][np.flatnonzero((m["program_op"] & 0xFF) == control_model.OP_SYMBOL)[0]] = control_model.OP_SYMBOL | (21 << 8)

    refused(fewer_slopes, "not its slopes plus one")
    refused(empty_ratio, "empty slope ratio")
    refused(no_profile, "without a parameter-profile transition")
    refused(special_with_ratio, "special-profile transition with a slope ratio")
    refused(pops_empty, "pops an empty stack")
    refused(bad_symbol, "formula symbol outside the list")
