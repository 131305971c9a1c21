#!/usr/bin/env python3
"""Generates tests/golden/targets5_golden.npz by running the REAL reference (build container only, after build()).

Per case of tests/targets5_cases.py the frames come from gvtm_targets_apply_host on a design-only model 5 plan of the class
(voice5_male.txt, 48 kHz), and go through oracle/_ref/ref_vtm as build() makes it, model "5" or "5f", control rate = the
plan's internal rate (one step per frame, frame s unchanged before step s) and poll=64: the model constructed with
interactive = true and driven as the editor's JACK callback drives it.  The drained samples are stored in full.  Two cases
are also stored through both models WITHOUT poll, the batch protocol's model on the same frames.

For every double-class case the second build of the reference (ref_vtm_o3) runs too and the two builds must agree under
parity_rules.check_model5, its 0.90 bit-identical share included: a case the reference's own builds do not keep inside the
bar the kernel is held to would have to be replaced, and the script stops there.

The moving average at the model 5 rate: tests/golden/ref_targets_table.cpp, unchanged and compiled as
make_targets_golden.py compiles it, on targets5_cases.FILTER_CASES at the plan's internal rate; the SHA-256 of its frames
is stored, so the filter at N = 3021 is pinned to the reference's MovingAverageFilter<float>.

    python tests/golden/make_targets5_golden.py
"""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import oracle  # noqa: E402
import parity_rules  # noqa: E402
import targets5_cases as cases  # noqa: E402
from gama_tts_amd import capi  # noqa: E402
from make_targets_golden import FLAGS, REF_VTM  # noqa: E402
from voice_cases import model5_plan  # noqa: E402


def reference(frames, float_class, rate, kind="gold", poll=cases.POLL):
    audio, info = oracle.ref_synthesize(frames, cases.MODEL[float_class], cases.RATE, rate, oracle.VOICE5_MALE, kind, poll=poll)
    assert int(info["steps"]) == frames.shape[0]
    return audio


def filter_shas(rate):
    keys = sorted(cases.FILTER_CASES)
    blob = [b"GVTI", struct.pack("<ii", 1, len(keys))]
    for key in keys:
        n_steps, lists = cases.filter_case(key)
        blob.append(struct.pack("<dq", rate, n_steps))
        for steps, values in lists:
            blob.append(struct.pack("<i", len(steps)))
            blob.append(np.asarray(steps, dtype="<i4").tobytes())
            blob.append(np.asarray(values, dtype="<f4").tobytes())
    with tempfile.TemporaryDirectory() as td:
        exe, pin, pout = os.path.join(td, "ref_targets_table"), os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        subprocess.run(["g++"] + FLAGS + ["-I" + REF_VTM, "-o", exe, os.path.join(HERE, "ref_targets_table.cpp")], check=True)
        with open(pin, "wb") as f:
            f.write(b"".join(blob))
        subprocess.run([exe, pin, pout], check=True)
        data = open(pout, "rb").read()
    assert data[:4] == b"GVTO" and struct.unpack_from("<ii", data, 4) == (1, len(keys))
    off, out = 12, {}
    for key in keys:
        n_steps = cases.FILTER_CASES[key]
        got = np.frombuffer(data, dtype="<f4", count=n_steps * 16, offset=off).reshape(n_steps, 16)
        off += got.size * 4
        out[key + "__sha256"] = np.frombuffer(cases.sha256_of_frames(got).encode(), dtype=np.uint8)
    assert off == len(data)
    return out


def main():
    out = {}
    for float_class in (True, False):
        plan = model5_plan(device=capi.DEVICE_NONE, float_class=float_class)
        rate = plan.info.internal_rate_hz
        assert plan.targets_filter_length() == cases.N and plan.info.output_rate == cases.RATE
        if not float_class:
            out.update(filter_shas(rate))
        for n_steps in cases.class_counts(float_class):
            frames = cases.frames_of(plan, n_steps)
            if n_steps > 1000:
                assert np.unique(frames[:, 0]).size > n_steps // 2, "the pitch must move"
            got = reference(frames, float_class, rate)
            assert got.size == plan.targets_output_count(n_steps), (n_steps, got.size)
            if not float_class:
                parity_rules.check_model5(reference(frames, float_class, rate, "o3"), got)  # (a case that fails here is replaced)
            key = cases.name(float_class, n_steps)
            out[key] = got
            out[key + "__frames"] = np.frombuffer(cases.sha256_of_frames(frames).encode(), dtype=np.uint8)
            if n_steps in cases.PLAIN:
                plain = reference(frames, float_class, rate, poll=0)
                assert plain.size == got.size
                out[cases.name(float_class, n_steps, plain=True)] = plain
            print(key, got.size, "samples")
    path = os.path.join(HERE, "targets5_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 600 * 1024


if __name__ == "__main__":
    main()
