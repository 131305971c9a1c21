#!/usr/bin/env python3
"""Generates tests/golden/targets_golden.npz by running the REAL reference's filter (build container only).

tests/golden/ref_targets_table.cpp is compiled here against /root/reference's vtm/MovingAverageFilter.h, included
unchanged, with -std=c++17 -O2 -ffp-contract=off, into a temporary directory outside the repository, and fed the cases of
tests/targets_cases.py.  The driver runs 16 MovingAverageFilter<float> of 50 ms under the loop of the rule as
include/gama_vtm.h states it: the editor's interactive window, whose behaviour that rule states, is a JACK client, and JACK
is not here.  The .npz holds data only, and little of it: per case the SHA-256 of its inputs, the SHA-256 of the [S][16]
float32 result, and the result itself where S <= 256.

    python tests/golden/make_targets_golden.py
"""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import targets_cases as cases  # noqa: E402

REF_VTM = os.path.join("/root/reference", "gama_tts", "src", "vtm")
FLAGS = ["-std=c++17", "-O2", "-ffp-contract=off", "-DNDEBUG", "-Wall"]


def main():
    names = list(cases.CASES)
    inputs = {n: cases.case(n) for n in names}
    blob = [b"GVTI", struct.pack("<ii", 1, len(names))]
    for n in names:
        key, n_steps, lists = inputs[n]
        blob.append(struct.pack("<dq", cases.PLANS[key].rate, n_steps))
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
    assert data[:4] == b"GVTO" and struct.unpack_from("<ii", data, 4) == (1, len(names))
    off = 12
    out = {}
    for n in names:
        key, n_steps, lists = inputs[n]
        got = np.frombuffer(data, dtype="<f4", count=n_steps * 16, offset=off).reshape(n_steps, 16).copy()
        off += got.size * 4
        out[n + "__inputs"] = np.frombuffer(cases.sha256_of_inputs(cases.PLANS[key].rate, n_steps, lists).encode(), dtype=np.uint8)
        out[n + "__sha256"] = np.frombuffer(cases.sha256_of_frames(got).encode(), dtype=np.uint8)
        if n_steps <= cases.FULL_ARRAY_STEPS:
            out[n + "__frames"] = got
        print(n, n_steps, "steps ->", cases.sha256_of_frames(got)[:16])
    assert off == len(data)
    path = os.path.join(HERE, "targets_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
