"""Model 5 under the interactive window on the device (gvtm_synthesize_targets_model5_device; vtm5_synth_kernel's targets
variant, csrc/vtm_kernels_m5t.hip and csrc/vtm_kernels_m5ft.hip, behind the check kernel).

The bar is the real reference constructed with interactive = true (tests/golden/targets5_golden.npz, made by
tests/golden/make_targets5_golden.py from oracle/_ref/ref_vtm with poll=64): the float class bit for bit against
VocalTractModel5<float,1>, the double class to parity_rules.check_model5 against VocalTractModel5<double,1>, in every shape
the variant has (float: chunk 60 and chunk 52; double: one utterance per workgroup, chunk 56, and two, chunk 24), at step
counts around a block of four, the chunk and the filter length (3021).  Counts exact, maxabs the largest sample, the audio
buffers start as a guard pattern and everything behind a row's count must still be the pattern.  Lists shared through list
ids, a refused utterance of every status between good ones, and the optional arguments left out."""
import os

import numpy as np
import pytest

import oracle
import targets5_cases as cases
from parity_rules import check_batch
from targets_io import guard_behind_counts, run_targets
from voice_cases import model5_plan

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(oracle.GOLDEN_DIR, "targets5_golden.npz"))


def check_against_fixture(fixture, plan, float_class, step_counts):
    audio, counts, maxabs, statuses = run_targets(plan, [cases.lists_of(s) for s in step_counts], step_counts)
    assert not statuses.any()
    refs = [fixture[cases.name(float_class, s)] for s in step_counts]
    for s, ref in zip(step_counts, refs):
        assert ref.size == plan.targets_output_count(s)
    check_batch(audio, counts, maxabs, refs, float_class)
    assert guard_behind_counts(audio, counts)
    return audio, counts, maxabs


def batches(chunk):
    """Batches of 1, 1, 3 and 9 that cover the step counts of a chunk."""
    r = cases.step_counts(chunk)
    return [r[10]], [r[8]], [r[0], r[13], r[7]], [r[1], r[2], r[3], r[4], r[5], r[6], r[9], r[11], r[12]]


# ---- a. the float class, bit-identical, both shapes ----

@pytest.mark.parametrize("rows,chunk", [(1, 60), (2, 52)])
def test_float_class_is_bit_identical_in_both_shapes(fixture, rows, chunk):
    plan = model5_plan(rows=rows, float_class=True)
    assert plan.targets_filter_length() == cases.N and cases.CHUNKS[True][rows - 1] == chunk
    for step_counts in batches(chunk):
        check_against_fixture(fixture, plan, True, step_counts)


def test_float_class_unforced_is_the_first_shape(fixture):
    # (up to one workgroup per compute unit: index 0, whose bytes the forced plan's are)
    plan = model5_plan(float_class=True)
    check_against_fixture(fixture, plan, True, [cases.N + 60, 61, 5])


# ---- b. the double class, one and two utterances per workgroup ----

@pytest.mark.parametrize("rows,chunk", [(1, 56), (2, 24)])
def test_double_class_against_the_reference(fixture, rows, chunk):
    plan = model5_plan(rows=rows)
    assert plan.targets_filter_length() == cases.N and cases.CHUNKS[False][rows - 1] == chunk
    # (odd batches: in the two-utterance shape the last workgroup runs half empty)
    for step_counts in batches(chunk):
        check_against_fixture(fixture, plan, False, step_counts)


def test_double_class_two_rows_equal_one_row(fixture):
    step_counts = [cases.N + 24, 51, 0, 25, 2 * cases.N + 24 + 5]
    utterances = [cases.lists_of(s) for s in step_counts]
    one = run_targets(model5_plan(rows=1), utterances, step_counts)
    two = run_targets(model5_plan(rows=2), utterances, step_counts)
    assert one[1].tolist() == two[1].tolist() and one[0].tobytes() == two[0].tobytes() and one[2].tobytes() == two[2].tobytes()


# ---- c. the samples are not the batch protocol's ----

def test_samples_are_the_interactive_models_not_the_batch_protocols(fixture):
    plan = model5_plan(float_class=True)
    for s in cases.PLAIN:
        audio, counts, _, _ = run_targets(plan, [cases.lists_of(s)], [s])
        got = audio[0, : counts[0]]
        assert got.tobytes() == fixture[cases.name(True, s)].tobytes()
        assert got.tobytes() != fixture[cases.name(True, s, plain=True)].tobytes()


# ---- d. shared lists ----

@pytest.mark.parametrize("float_class", [True, False], ids=["float", "double"])
def test_shared_lists_give_the_bytes_of_lists_of_their_own(float_class):
    plan = model5_plan(float_class=float_class)
    shared = cases.lists_of(cases.N)
    moved = [cases.targets_cases.spoken_lists(700, 10 + b)[9] for b in range(8)]  # r3, one list per utterance: fifteen are shared
    step_counts = [700, 650, 700, 1, 333, 700, 0, 512]
    ids = [[16 + b if p == 9 else p for p in range(16)] for b in range(8)]
    a = run_targets(plan, shared + moved, step_counts, ids=ids, max_steps=700)
    own = [[moved[b] if p == 9 else shared[p] for p in range(16)] for b in range(8)]
    b = run_targets(plan, own, step_counts, max_steps=700)
    assert not a[3].any() and not b[3].any()
    assert a[0].tobytes() == b[0].tobytes() and a[1].tolist() == b[1].tolist() and a[2].tobytes() == b[2].tobytes()
    assert guard_behind_counts(a[0], a[1])
    assert len({a[0][i, : a[1][i]].tobytes() for i in (0, 2, 5)}) == 3  # (the one parameter that differs is heard)


# ---- e. statuses ----

@pytest.mark.parametrize("float_class,rows", [(True, 0), (False, 2)], ids=["float", "double-two-rows"])
def test_a_refused_utterance_of_every_status_between_good_ones(float_class, rows):
    plan = model5_plan(float_class=float_class, rows=rows)
    good = lambda seed: cases.targets_cases.spoken_lists(400, seed)  # noqa: E731

    def with_list(seed, p, steps, values):
        lists = good(seed)
        lists[p] = (steps, np.asarray(values, dtype=np.float32))
        return lists

    utterances = [good(0), good(1), good(2), with_list(3, 4, [0, 9], [1.0, np.nan]), good(4), with_list(5, 15, [0, 7], [1.0, np.inf]),
                  with_list(6, 2, [5, 5], [1.0, 2.0]), good(7), with_list(8, 0, [-1], [1.0]), with_list(9, 3, [9, 4], [-np.inf, 2.0]), good(10),
                  good(11), good(12)]
    step_counts = [400, -1, 401, 300, 250, 300, 300, 1, 300, 300, 300, 400, 77]
    want = [0, 1, 1, 3, 0, 3, 4, 0, 4, 3, 2, 1, 0]
    ids = np.arange(13 * 16, dtype=np.int32).reshape(13, 16)
    ids[11, 6] = 13 * 16  # a list id outside the table

    def doctor(offsets, steps, values):
        offsets[10 * 16 + 3] = offsets[10 * 16 + 4] + 1  # utterance 10's list 3 ends before it begins

    lists = [l for u in utterances for l in u]
    audio, counts, maxabs, statuses = run_targets(plan, lists, step_counts, ids=ids, max_steps=400, doctor=doctor)
    assert statuses.tolist() == want
    zero = plan.targets_output_count(0)
    assert all(counts[b] == (plan.targets_output_count(step_counts[b]) if want[b] == 0 else zero) for b in range(13))
    assert guard_behind_counts(audio, counts)
    # the good utterances' bytes are those of the same batch without the refused ones
    keep = [b for b in range(13) if want[b] == 0]
    alone = run_targets(plan, [utterances[b] for b in keep], [step_counts[b] for b in keep], max_steps=400)
    assert not alone[3].any()
    for i, b in enumerate(keep):
        assert alone[1][i] == counts[b] and alone[2][i].tobytes() == maxabs[b].tobytes()
        assert alone[0][i, : counts[b]].tobytes() == audio[b, : counts[b]].tobytes(), b
    # a refused utterance is one of 0 steps
    empty = run_targets(plan, [good(0)], [0], max_steps=400)
    for b in range(13):
        if want[b]:
            assert audio[b, :zero].tobytes() == empty[0][0, :zero].tobytes() and maxabs[b] == empty[2][0]
    # no status asked for: the same audio
    silent = run_targets(plan, lists, step_counts, ids=ids, max_steps=400, doctor=doctor, status=False)
    assert silent[0].tobytes() == audio.tobytes() and (silent[3] == -9).all()
    # nothing to do
    assert plan._lib.gvtm_synthesize_targets_model5_device(plan._h, None, 0, None, None, None, None, 0, 0, None, 0, None, None, None, None) == 0


# ---- f. the optional arguments ----

def test_null_step_counts_and_null_outputs(fixture):
    plan = model5_plan(float_class=True)
    s = 2 * 52 + 3
    utterances = [cases.lists_of(s)] * 3
    full = run_targets(plan, utterances, [s] * 3)
    assert full[0][0, : full[1][0]].tobytes() == fixture[cases.name(True, s)].tobytes()
    # d_step_counts == NULL: every utterance has max_steps steps
    every = run_targets(plan, utterances, [s] * 3, steps_in=False)
    assert every[0].tobytes() == full[0].tobytes() and every[1].tolist() == full[1].tolist() and every[2].tobytes() == full[2].tobytes()
    # no status, no peaks, no counts: the same samples, the fills untouched
    bare = run_targets(plan, utterances, [s] * 3, status=False, peaks=False, counts=False)
    assert bare[0].tobytes() == full[0].tobytes()
    assert (bare[1] == -7).all() and (bare[2] == 5.0).all() and (bare[3] == -9).all()
