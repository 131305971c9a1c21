#!/usr/bin/env python3
"""Generates tests/golden/targets5_voices_golden.npz by running the REAL reference (build container only, after build()).

Made the way make_targets5_golden.py makes targets5_golden.npz, for the four voices that file lacks.  Per case of
tests/targets5_voices_cases.py the frames come from gvtm_targets_apply_host(plan, voice = v) on a design-only plan of all
five model 5 voices of the class (48 kHz), and go through oracle/_ref/ref_vtm as build() makes it, model "5" or "5f", the
voice's own file, control rate = the voice's internal rate (one step per frame) and poll=64: the model constructed with
interactive = true and driven as the editor's JACK callback drives it.  The drained samples are stored in full, with the
SHA-256 of the frames they were made from.

For every double-class case the second build of the reference (ref_vtm_o3) runs too and the two builds must agree under
parity_rules.check_model5, its bit-identical share included: a case that fails there is replaced, not loosened.

    python tests/golden/make_targets5_voices_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import oracle  # noqa: E402
import parity_rules  # noqa: E402
import targets5_voices_cases as cases  # noqa: E402
from voice_files import VOICES, voice_path  # noqa: E402


def reference(frames, float_class, voice, rate, kind="gold"):
    audio, info = oracle.ref_synthesize(frames, cases.MODEL[float_class], cases.RATE, rate, voice_path(voice, True), kind, poll=cases.POLL)
    assert int(info["steps"]) == frames.shape[0]
    return audio


def main():
    out = {}
    for float_class in (True, False):
        plan = cases.voices_plan(float_class)
        lengths = [plan.targets_filter_length(v) for v in range(plan.n_voices)]
        assert lengths[0] == cases.MALE_N and len(set(lengths)) == 5 and plan.info.output_rate == cases.RATE
        for voice, n_steps in cases.all_cases(plan, float_class):
            v = VOICES.index(voice)
            rate = plan.voice_info(v).internal_rate_hz
            frames = cases.frames_of(plan, voice, n_steps)
            if n_steps > 1000:
                assert np.unique(frames[:, 0]).size > n_steps // 2, "the pitch must move"
            got = reference(frames, float_class, voice, rate)
            assert got.size == plan.targets_voice_output_count(v, n_steps), (voice, n_steps, got.size)
            if not float_class:
                parity_rules.check_model5(reference(frames, float_class, voice, rate, "o3"), got)  # (a case that fails here is replaced)
            key = cases.name(float_class, voice, n_steps)
            out[key] = got
            out[key + "__frames"] = np.frombuffer(cases.sha256_of_frames(frames).encode(), dtype=np.uint8)
            print(key, got.size, "samples")
    path = os.path.join(HERE, "targets5_voices_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 600 * 1024


if __name__ == "__main__":
    main()
