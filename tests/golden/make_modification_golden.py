#!/usr/bin/env python3
"""Generates tests/golden/modification_golden.npz by running the REAL reference's filter (build container only).

tests/golden/ref_modification_table.cpp is compiled here against /root/reference's vtm/MovingAverageFilter.h, included
unchanged, with -std=c++17 -O2 -ffp-contract=off, into a temporary directory outside the repository, and fed the cases of
tests/modification_cases.py.  The driver runs MovingAverageFilter<float> under the loop of the rule as include/gama_vtm.h
states it (frames, steps, the point at step s, the frame's first step): the editor's processor, whose behaviour that rule
states, is a JACK client, and JACK is not here.  The .npz holds data only: per case the SHA-256 of its inputs, the internal rate and control steps it was run at, and the
columns of the modified list that its gestures name.

    python tests/golden/make_modification_golden.py
"""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import modification_cases as cases  # noqa: E402

REF_VTM = os.path.join("/root/reference", "gama_tts", "src", "vtm")
FLAGS = ["-std=c++17", "-O2", "-ffp-contract=off", "-DNDEBUG", "-Wall"]


def main():
    names = list(cases.CASES)
    inputs = {n: cases.case(n) for n in names}
    blob = [b"GVMI", struct.pack("<ii", 1, len(names))]
    for n in names:
        key, frames, gestures = inputs[n]
        plan = cases.PLANS[key]
        blob.append(struct.pack("<dii", plan.rate, plan.cs, frames.shape[0]))
        blob.append(np.ascontiguousarray(frames, dtype="<f4").tobytes())
        blob.append(struct.pack("<i", len(gestures)))
        for p, op, steps, values in gestures:
            blob.append(struct.pack("<iii", p, op, len(steps)))
            blob.append(np.asarray(steps, dtype="<i4").tobytes())
            blob.append(np.asarray(values, dtype="<f4").tobytes())
    with tempfile.TemporaryDirectory() as td:
        exe, pin, pout = os.path.join(td, "ref_modification_table"), os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        subprocess.run(["g++"] + FLAGS + ["-I" + REF_VTM, "-o", exe, os.path.join(HERE, "ref_modification_table.cpp")], check=True)
        with open(pin, "wb") as f:
            f.write(b"".join(blob))
        subprocess.run([exe, pin, pout], check=True)
        data = open(pout, "rb").read()
    assert data[:4] == b"GVMO" and struct.unpack_from("<ii", data, 4) == (1, len(names))
    off = 12
    out = {}
    for n in names:
        key, frames, gestures = inputs[n]
        got = np.frombuffer(data, dtype="<f4", count=frames.size, offset=off).reshape(frames.shape).copy()
        off += frames.size * 4
        columns = cases.modified_parameters(gestures)
        untouched = [c for c in range(16) if c not in columns]
        assert got[:, untouched].tobytes() == frames[:, untouched].tobytes() and got[:1].tobytes() == frames[:1].tobytes(), n
        out[n + "__sha256"] = np.frombuffer(cases.sha256_of(frames, gestures).encode(), dtype=np.uint8)
        out[n + "__plan"] = np.array([cases.PLANS[key].rate, cases.PLANS[key].cs], dtype=np.float64)
        out[n + "__columns"] = got[:, columns].copy()
        print(n, frames.shape[0], "frames", len(gestures), "gestures ->", int((got.view(np.uint32) != frames.view(np.uint32)).sum()), "values modified")
    assert off == len(data)
    path = os.path.join(HERE, "modification_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
