#!/usr/bin/env python3
"""Generates tests/golden/intonation_golden.npz by running the REAL reference (build container only).

tests/golden/ref_intonation_table.cpp is compiled here against /root/reference with the whole-library flags of
oracle/Makefile (-std=c++17 -O2 -ffp-contract=off), into a temporary directory outside the repository, and fed the cases
of tests/intonation_cases.py: per case the reference's own clearMacroIntonation(), prepareMacroIntonationInterpolation()
and generateOutput().  The .npz holds data only: per case the SHA-256 of its inputs, time, has_interp and interp[4] of
every merged event, the SHA-256 of the whole merged table, the frame count and the frames (longer cases: the SHA-256 of
the frames and every FRAME_STRIDE-th frame).

    python tests/golden/make_intonation_golden.py
"""
import glob
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import intonation_cases as cases  # noqa: E402

REF = "/root/reference"
REF_SRC = os.path.join(REF, "gama_tts", "src")
REF_VOICE_DIR = os.path.join(REF, "data", "voice", "english", "0_male")
FLAGS = ["-std=c++17", "-O2", "-ffp-contract=off", "-DENABLE_VTM_PLUGINS=1", "-DNDEBUG", "-w"]
INCLUDES = ["-I" + os.path.join(REF_SRC, d) for d in ("", "rapidxml", "text_parser", "vtm", "vtm_control_model", "xml")]


def build(workdir):
    """The reference's translation units (all but main.cpp) and ref_intonation_table.cpp -> workdir/ref_intonation_table"""
    sources = [s for s in glob.glob(os.path.join(REF_SRC, "**", "*.cpp"), recursive=True) if os.path.basename(s) != "main.cpp"]
    objects = []
    jobs = []
    for i, src in enumerate(sorted(sources)):
        obj = os.path.join(workdir, "%03d.o" % i)
        objects.append(obj)
        jobs.append(subprocess.Popen(["g++"] + FLAGS + INCLUDES + ["-c", "-o", obj, src]))
        if len(jobs) == 8:
            assert jobs.pop(0).wait() == 0
    for j in jobs:
        assert j.wait() == 0
    exe = os.path.join(workdir, "ref_intonation_table")
    subprocess.run(["g++"] + FLAGS + INCLUDES + ["-o", exe, os.path.join(HERE, "ref_intonation_table.cpp")] + objects + ["-ldl"], check=True)
    return exe


def main():
    golden_tracks = dict(np.load(os.path.join(HERE, "tracks_golden.npz")))
    base_tables = cases.bases(golden_tracks)
    names = list(cases.CASES)
    inputs = {n: cases.case(n, base_tables) for n in names}
    blob = [b"GVII", struct.pack("<ii", 1, len(names))]
    for n in names:
        table, points, c = inputs[n]
        blob.append(struct.pack("<i", table.shape[0]))
        blob.append(np.ascontiguousarray(table, dtype="<f8").tobytes())
        blob.append(struct.pack("<i", points.shape[0]))
        blob.append(np.ascontiguousarray(points, dtype="<f8").tobytes())
        blob.append(struct.pack("<5i5d", *(int(x) for x in c[:5]), *(float(x) for x in c[5:10])))
    with tempfile.TemporaryDirectory() as td:
        exe = build(td)
        pin, pout = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        with open(pin, "wb") as f:
            f.write(b"".join(blob))
        subprocess.run([exe, REF_VOICE_DIR, pin, pout], check=True)
        data = open(pout, "rb").read()
    assert data[:4] == b"GVIO" and struct.unpack_from("<ii", data, 4) == (1, len(names))
    off = 12
    out = {}
    for n in names:
        table, points, c = inputs[n]
        (m,) = struct.unpack_from("<i", data, off)
        off += 4
        merged = np.frombuffer(data, dtype="<f8", count=m * 38, offset=off).reshape(m, 38).copy()
        off += m * 38 * 8
        (nf,) = struct.unpack_from("<i", data, off)
        off += 4
        frames = np.frombuffer(data, dtype="<f4", count=nf * 16, offset=off).reshape(nf, 16).copy()
        off += nf * 64
        out[n + "__base_sha256"] = np.frombuffer(cases.sha256(table, "<f8").encode(), dtype=np.uint8)
        out[n + "__points_sha256"] = np.frombuffer(cases.sha256(points, "<f8").encode(), dtype=np.uint8)
        out[n + "__cfg"] = np.asarray(c, dtype=np.float64)
        out[n + "__time"] = merged[:, 0].astype(np.int32)
        out[n + "__has_interp"] = merged[:, 1].astype(np.int8)
        out[n + "__interp"] = merged[:, 2:6].copy()
        out[n + "__sha256"] = np.frombuffer(cases.sha256(merged, "<f8").encode(), dtype=np.uint8)
        out[n + "__count"] = np.int64(nf)
        if nf <= cases.FULL_FRAMES:
            out[n + "__frames"] = frames
        else:
            out[n + "__frames_sha256"] = np.frombuffer(cases.sha256(frames, "<f4").encode(), dtype=np.uint8)
            out[n + "__strided"] = frames[:: cases.FRAME_STRIDE].copy()
        print(n, table.shape[0], "events", points.shape[0], "points ->", m, "merged,", nf, "frames")
    assert off == len(data)
    path = os.path.join(HERE, "intonation_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
