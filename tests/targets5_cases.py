"""The cases of tests/golden/targets5_golden.npz: reference model 5 as the editor's interactive window runs it --
VocalTractModel5<T,1>(config, interactive = true), which divides each step's signal by that step's f0
(vtm/VocalTractModel5.h:579) -- fed the frames gvtm_targets_apply_host makes of spoken target lists
(targets_cases.spoken_lists) by setParameter before every step, then finishSynthesis().  The voice is 5_male
(tests/golden/voice5_male.txt) at 48 kHz, whose internal rate gives a filter of N = 3021 samples.

A case is a step count S: its lists are spoken_lists(LONGEST, seed), the same whatever S, with a seed of its own; some cases
carry wide values, on fricCF and fricBW only and positive.  The pitch list moves (a point every 211 steps through a window of
3021), so f0 differs from step to step in every case longer than a few hundred steps.  The step counts are the issue's, C
running over the chunk of every shape of the kernel's targets variant (csrc/vtm_kernel_m5.inc: m5_targets_shape): the float
class's 60 and 52, stored from the reference's float class ("5f"), and the double class's 56 and 24, stored from its double
class ("5")."""
import hashlib

import numpy as np

import targets_cases

RATE = 48000.0
N = 3021          # gvtm_targets_filter_length of the plan (internal rate 60 411.43 Hz)
LONGEST = 6200    # steps the lists are made for: beyond 2 N + 60 + 5
POLL = 64         # samples per callback of the reference's interactive driver (oracle/ref_driver.cpp: poll=<n>)
# chunk of the shape a diagnostics plan forces with rows 1 / rows 2, by class (float: index 0 / 1; double: one / two utterances)
CHUNKS = {True: (60, 52), False: (56, 24)}
MODEL = {True: "5f", False: "5"}


def step_counts(chunk, n=N):
    """The step counts an utterance can go wrong at: around a block of four, the chunk and the filter length."""
    return [0, 1, 3, 4, 5, chunk - 1, chunk, chunk + 1, 2 * chunk + 3, n - 1, n, n + 1, n + chunk, 2 * n + chunk + 5]


# the two cases whose frames are also stored through the model as the batch protocol constructs it (interactive = false),
# in both classes
PLAIN = (N + 60, 2 * 24 + 3)


def class_counts(float_class):
    """Every step count the fixture holds for a class, ascending."""
    return sorted({s for c in CHUNKS[float_class] for s in step_counts(c)} | set(PLAIN))


ALL_COUNTS = sorted(set(class_counts(True)) | set(class_counts(False)))
SEED = {s: i for i, s in enumerate(ALL_COUNTS)}       # a case's seed: its place among all step counts
WIDE = {s for i, s in enumerate(ALL_COUNTS) if i % 3 == 2}  # every third case: fricCF / fricBW six decades apart in one window


def name(float_class, n_steps, plain=False):
    return "%s__s%d%s" % (MODEL[float_class], n_steps, "__plain" if plain else "")


def lists_of(n_steps):
    """The 16 lists of case S: (steps, values) each."""
    return targets_cases.spoken_lists(LONGEST, 100 + SEED[n_steps], wide=n_steps in WIDE)


def frames_of(plan, n_steps):
    """gvtm_targets_apply_host's frames of case S under the plan's filter -> float32 [S][16]."""
    from gama_tts_amd import capi
    frames, status = capi.targets_apply_host(plan, lists_of(n_steps), n_steps)
    assert status == 0
    return frames


def sha256_of_frames(frames):
    return hashlib.sha256(np.ascontiguousarray(frames, dtype="<f4").tobytes()).hexdigest()


# ---- the moving average at the model 5 rate, pinned to the reference's MovingAverageFilter<float> ----
# (tests/golden/ref_targets_table.cpp, unchanged, run at the plan's internal rate on targets_cases.standard_lists: every kind
# of list the rule distinguishes, at a window of 3021 samples)
FILTER_CASES = {"n5__s1": 1, "n5__nm1": N - 1, "n5__np1": N + 1, "n5__2n7": 2 * N + 7}


def filter_case(key):
    """-> (S, 16 lists) of a filter case"""
    n_steps = FILTER_CASES[key]
    return n_steps, targets_cases.standard_lists(N, n_steps, 500 + sorted(FILTER_CASES).index(key))
