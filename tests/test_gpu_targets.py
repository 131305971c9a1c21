"""Synthesis from parameter targets on the device (gvtm_synthesize_targets_device; the targets driver of vtm_synth_kernel
and the check kernel in front of it, csrc/vtm_kernels_targets.hip).

The bar is the header's tie: the samples are those of the host rule's frames (gvtm_targets_apply_host) synthesized at one
step per frame.  Float: bit-identical to the oracle's float class at control rate = internal rate, in every row count, at
step counts around the chunk and the filter length, and byte for byte what gvtm_synthesize_batch_device gives today on a
plan of control_steps == 1 fed those frames.  fp64 and mixed: the project's own bars (parity_rules.TOL).  Lists shared through
list ids, a refused utterance of every status between good ones (the audio buffers start as a guard pattern and everything
behind a row's count must still be the pattern), and the plans the entry does not take.

The lists are spoken (targets_cases.spoken_lists): key values of a random utterance at steps that are multiples of nothing in
the kernel; wide values (six decades apart in one window) go on fricCF and fricBW only, positive."""
import ctypes

import numpy as np
import pytest

import gama_tts_amd as g
from gama_tts_amd import capi
import oracle
import targets_cases as cases
from device_io import current_stream, filled, to_device, to_host
from parity_rules import TOL, check_batch, within
from targets_io import GUARD, guard_behind_counts, run_targets
from voice_cases import configs, male_plan, model5_plan

pytestmark = pytest.mark.gpu

UNSUPPORTED = 4
LONGEST = 6200  # steps the host rule's frames are made for, once per utterance: a shorter utterance's are their first rows


def chunk_of(plan, batch):
    return int(plan._lib.gvtm_debug_chunk_length(plan._h, batch))


def ragged(chunk, n):
    """The step counts an utterance can go wrong at: around a block of four, the chunk and the filter length."""
    return [0, 1, 3, 4, 5, chunk - 1, chunk, chunk + 1, 2 * chunk + 3, n - 1, n, n + 1, n + chunk, 3 * n + chunk + 5]


_frames = {}


def host_frames(plan, key, seed, n_steps, wide=False):
    """gvtm_targets_apply_host's frames for utterance `seed` under the plan's filter, computed once for LONGEST steps."""
    if (key, seed, wide) not in _frames:
        lists = cases.spoken_lists(LONGEST, seed, wide=wide)
        frames, status = capi.targets_apply_host(plan, lists, LONGEST)
        assert status == 0
        _frames[key, seed, wide] = (lists, frames)
    lists, frames = _frames[key, seed, wide]
    return lists, frames[:n_steps]


def oracle_refs(plan, cfg, key, seeds, step_counts, wide=False):
    rate = plan.info.internal_rate_hz
    assert oracle.derive(cfg, rate).control_steps == 1
    return [oracle.synthesize(cfg, host_frames(plan, key, seed, s, wide)[1], control_rate=rate) for seed, s in zip(seeds, step_counts)]


def check_float(plan, cfg, key, step_counts, wide=False):
    seeds = list(range(len(step_counts)))
    utterances = [host_frames(plan, key, seed, s, wide)[0] for seed, s in zip(seeds, step_counts)]
    audio, counts, maxabs, statuses = run_targets(plan, utterances, step_counts)
    assert not statuses.any()
    refs = oracle_refs(plan, cfg, key, seeds, step_counts, wide)
    for b, s in enumerate(step_counts):
        assert refs[b].size == plan.targets_output_count(s)
    check_batch(audio, counts, maxabs, refs, True)
    assert guard_behind_counts(audio, counts)
    return audio, counts, maxabs


# ---- a. float, bit-identical, every row count ----

@pytest.mark.parametrize("rows,chunk", [(1, 144), (2, 96), (4, 48)])
def test_float_is_bit_identical_in_every_row_count(rows, chunk):
    plan = male_plan(precision=capi.PRECISION_F32, rows=rows)
    n = plan.targets_filter_length()
    assert (chunk_of(plan, 9), n) == (chunk, 1002)
    cfg = oracle.male_config(44100.0, 1, float_model=1)
    r = ragged(chunk, n)
    # batches of 1, 3 and 9: some rows of a workgroup stay empty; between them every step count of the rule
    for step_counts in ([r[10]], [r[8]], [r[0], r[13], r[7]], [r[1], r[2], r[3], r[4], r[5], r[6], r[9], r[11], r[12]]):
        check_float(plan, cfg, "male", step_counts, wide=len(step_counts) == 3)


# ---- b. the same bytes as today's route ----

def test_float_equals_the_batch_entry_at_one_step_per_frame():
    plan = male_plan(precision=capi.PRECISION_F32)
    n, chunk = plan.targets_filter_length(), 144
    step_counts = [ragged(chunk, n)[i] for i in (1, 3, 5, 6, 7, 8, 10, 12, 13)]
    seeds = list(range(9))
    utterances = [host_frames(plan, "male", seed, s)[0] for seed, s in zip(seeds, step_counts)]
    audio, counts, maxabs, _ = run_targets(plan, utterances, step_counts)
    rate = plan.info.internal_rate_hz
    today = male_plan(precision=capi.PRECISION_F32, crate=rate)
    assert today.info.control_steps == 1 and today.info.internal_rate_hz == rate
    max_steps = max(step_counts)
    stride = today.output_capacity(max_steps)
    assert stride == plan.targets_output_capacity(max_steps) == audio.shape[1]
    params = np.zeros((9, max_steps, 16), np.float32)
    for b, (seed, s) in enumerate(zip(seeds, step_counts)):
        params[b, :s] = host_frames(plan, "male", seed, s)[1]
    d_params, d_frames = to_device(params, np.asarray(step_counts, dtype=np.int32))
    d_audio, d_counts, d_maxabs = filled((9, stride * 4), GUARD, np.uint8), filled(9, -7, np.int64), filled(9, 5.0, np.float32)
    today.synthesize_device(d_params, 9, max_steps, d_audio, stride, d_frames, d_counts, d_maxabs, current_stream())
    t_audio, t_counts, t_maxabs = to_host(d_audio, d_counts, d_maxabs)
    assert t_counts.tolist() == counts.tolist() and t_maxabs.tobytes() == maxabs.tobytes()
    t_audio = t_audio.view(np.float32).reshape(9, stride)
    for b in range(9):
        assert t_audio[b, : counts[b]].tobytes() == audio[b, : counts[b]].tobytes(), b


# ---- c. float, SectionDelay 2 (running-remainder bounds, phase table), and a down-sampling plan ----

@pytest.mark.parametrize("rows,chunk", [(4, 48), (2, 96)])
def test_float_section_delay_2(rows, chunk):
    plan = male_plan(precision=capi.PRECISION_F32, delay=2, rows=rows)
    n = plan.targets_filter_length()
    assert (chunk_of(plan, 5), n) == (chunk, 2003)
    r = ragged(chunk, n)
    check_float(plan, oracle.male_config(44100.0, 2, float_model=1), "male-d2", [r[7], r[11], r[0], r[13], r[8]])


def test_float_down_sampling():
    plan = male_plan(precision=capi.PRECISION_F32, rate=16000.0)
    assert plan.info.internal_rate_hz > 16000.0
    audio, counts, _ = check_float(plan, oracle.male_config(16000.0, 1, float_model=1), "male-16k", [1002 + 145, 5])
    assert plan.targets_output_capacity(1147) > counts.max()  # (the 1024-sample ring's flush overrun: a shorter utterance may yield more)


# ---- d. fp64 and mixed against the oracle's double class ----

@pytest.mark.parametrize("precision", [capi.PRECISION_F64, capi.PRECISION_MIXED], ids=["f64", "mixed"])
@pytest.mark.parametrize("rows", [1, 4])
def test_double_classes_against_the_oracle(precision, rows):
    plan = male_plan(precision=precision, rows=rows)
    n, chunk = plan.targets_filter_length(), chunk_of(plan, 5)
    r = ragged(chunk, n)
    step_counts = [r[8], r[0], r[11], r[5], r[12]]
    seeds = list(range(5))
    # (the double classes' frames: the same float rule, under this plan's rate)
    utterances = [host_frames(plan, "male", seed, s)[0] for seed, s in zip(seeds, step_counts)]
    audio, counts, maxabs, statuses = run_targets(plan, utterances, step_counts)
    assert not statuses.any()
    refs = oracle_refs(plan, oracle.male_config(44100.0, 1), "male", seeds, step_counts)
    for b, ref in enumerate(refs):
        assert counts[b] == ref.size == plan.targets_output_count(step_counts[b])
        assert within(audio[b, : ref.size], ref, TOL[precision]), b
        assert maxabs[b] == (np.abs(audio[b, : ref.size]).max() if ref.size else 0.0)
    assert guard_behind_counts(audio, counts)


# ---- e. shared lists ----

def test_shared_lists_give_the_bytes_of_lists_of_their_own():
    plan = male_plan(precision=capi.PRECISION_F32)
    shared = cases.spoken_lists(700, 3)
    moved = [cases.spoken_lists(700, 10 + b)[9] for b in range(8)]  # r3, one list per utterance
    step_counts = [700, 650, 700, 1, 333, 700, 0, 512]
    ids = [[16 + b if p == 9 else p for p in range(16)] for b in range(8)]
    a = run_targets(plan, shared + moved, step_counts, ids=ids, max_steps=700)
    own = [[moved[b] if p == 9 else shared[p] for p in range(16)] for b in range(8)]
    b = run_targets(plan, own, step_counts, max_steps=700)
    assert not a[3].any() and not b[3].any()
    assert a[0].tobytes() == b[0].tobytes() and a[1].tolist() == b[1].tolist() and a[2].tobytes() == b[2].tobytes()
    assert len({a[0][i, : a[1][i]].tobytes() for i in (0, 2, 5)}) == 3  # (the one parameter that differs is heard)


# ---- f. statuses ----

def test_a_refused_utterance_of_every_status_between_good_ones():
    plan = male_plan(precision=capi.PRECISION_F32)
    good = lambda seed: cases.spoken_lists(400, seed)  # noqa: E731

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
    assert plan._lib.gvtm_synthesize_targets_device(plan._h, None, 0, None, None, None, None, 0, 0, None, 0, None, None, None, None) == 0


# ---- g. plans the entry does not take ----

def test_unsupported_plans():
    offsets, steps, values = capi.pack_targets(cases.spoken_lists(10, 0))
    d_offsets, d_steps, d_values = to_device(offsets, steps, values)
    for plan in (g.VoicesPlan(configs(44100.0, 1, capi.PRECISION_F32, names=["male", "female"]), 250.0, 0), model5_plan("male")):
        stride = plan.targets_output_capacity(10)
        d_audio = filled((1, stride), 0.0, np.float32)
        rc = plan._lib.gvtm_synthesize_targets_device(plan._h, capi._ptr(d_offsets), 16, None, capi._ptr(d_steps), capi._ptr(d_values), None, 1, 10,
                                                      capi._ptr(d_audio), stride, None, None, None, None)
        assert rc == UNSUPPORTED


# ---- h. eight rows forced ----

def test_forced_eight_rows_on_the_frames_and_the_targets_entry():
    """Eight utterances per workgroup are the one point where the variants of vtm_synth_kernel differ in their launch
    (csrc/vtm_kernel_shapes.hpp: launch_v2): the frames variant of one voice has the kernel, every other variant would refuse
    the shape with hipErrorInvalidValue ahead of any launch.  Through the C ABI that refusal is not reached: the eight-row
    shape of a float male plan needs 169 072 bytes of LDS, more than a workgroup has (160 KB), so the one row choice
    (synth_launch_shape) halves the forced rows for every entry alike.  Read on the build before launch_v2 became one
    function: the targets entry returns status 0 and synthesizes in four rows, as the frames entry does; this pins both,
    to the bytes of the one-row shape."""
    eight = male_plan(precision=capi.PRECISION_F32, rows=8)
    shape = (ctypes.c_size_t * 3)()
    assert eight._lib.gvtm_debug_launch_shape(eight._h, 2, 0, shape) == 0
    assert shape[0] == 4 and shape[2] <= 160 * 1024 < eight._lib.gvtm_debug_lds_bytes(eight._h, 8)
    step_counts = [24, 24]
    utterances = [host_frames(eight, "male", seed, 24)[0] for seed in (0, 1)]
    audio, counts, maxabs, statuses = run_targets(eight, utterances, step_counts)  # (raises on a status other than 0)
    one = run_targets(male_plan(precision=capi.PRECISION_F32), utterances, step_counts)
    assert not statuses.any() and not one[3].any()
    assert counts.tolist() == one[1].tolist() == [eight.targets_output_count(24)] * 2 and maxabs.tobytes() == one[2].tobytes()
    assert audio.tobytes() == one[0].tobytes() and guard_behind_counts(audio, counts)
    # the frames entry with eight rows forced, one step per frame: the same shape, the same bytes
    rate = eight.info.internal_rate_hz
    frames8 = male_plan(precision=capi.PRECISION_F32, crate=rate, rows=8)
    assert frames8.info.control_steps == 1 and chunk_of(frames8, 2) == chunk_of(eight, 2) == 48
    stride = frames8.output_capacity(24)
    assert stride == audio.shape[1]
    params = np.stack([host_frames(eight, "male", seed, 24)[1] for seed in (0, 1)]).astype(np.float32)
    d_params, d_frames = to_device(params, np.asarray(step_counts, dtype=np.int32))
    d_audio, d_counts, d_maxabs = filled((2, stride * 4), GUARD, np.uint8), filled(2, -7, np.int64), filled(2, 5.0, np.float32)
    frames8.synthesize_device(d_params, 2, 24, d_audio, stride, d_frames, d_counts, d_maxabs, current_stream())
    f_audio, f_counts, f_maxabs = to_host(d_audio, d_counts, d_maxabs)
    assert f_counts.tolist() == counts.tolist() and f_maxabs.tobytes() == maxabs.tobytes()
    f_audio = f_audio.view(np.float32).reshape(2, stride)
    for b in range(2):
        assert f_audio[b, : counts[b]].tobytes() == audio[b, : counts[b]].tobytes(), b
