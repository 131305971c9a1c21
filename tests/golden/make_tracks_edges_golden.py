#!/usr/bin/env python3
"""Generates tests/golden/tracks_edges_golden.npz by running the REAL reference (build container only).

oracle/_ref/ref_tracks_table (oracle/ref_tracks_table.cpp, compiled against /root/reference by `make -C oracle ref_full`)
feeds the event lists of tests/tracks_edges_cases.py to the reference's own EventList::generateOutput(), one EventList per
list, its calls one after the other (the drift generator runs on from call to call).  The .npz holds data only: per list
the SHA-256 of its table; per call the settings, the frame count and the frames (longer calls: the SHA-256 of the frames
and every FRAME_STRIDE-th frame).

    make -C oracle ref_full && python tests/golden/make_tracks_edges_golden.py
"""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oracle  # noqa: E402
import tracks_edges_cases as cases  # noqa: E402

REF_VOICE_DIR = "/root/reference/data/voice/english/0_male"


def main():
    golden_tracks = dict(np.load(os.path.join(HERE, "tracks_golden.npz")))
    names = list(cases.LISTS)
    tables = {n: cases.table(n, golden_tracks) for n in names}
    blob = [b"GVTI", struct.pack("<ii", 1, len(names))]
    for n in names:
        t = np.ascontiguousarray(tables[n], dtype="<f8")
        blob.append(struct.pack("<i", t.shape[0]))
        blob.append(t.tobytes())
        blob.append(struct.pack("<i", len(cases.calls(n))))
        for c in cases.calls(n):
            blob.append(struct.pack("<5i5d", *(int(x) for x in c[:5]), *(float(x) for x in c[5:10])))
    with tempfile.TemporaryDirectory() as td:
        pin, pout = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        with open(pin, "wb") as f:
            f.write(b"".join(blob))
        subprocess.run([os.path.join(oracle.REF_DIR, "ref_tracks_table"), REF_VOICE_DIR, pin, pout], check=True)
        data = open(pout, "rb").read()
    assert data[:4] == b"GVTO" and struct.unpack_from("<ii", data, 4) == (1, len(names))
    off = 12
    out = {}
    for n in names:
        out[n + "__table_sha256"] = np.frombuffer(cases.table_sha256(tables[n]).encode(), dtype=np.uint8)
        out[n + "__events"] = np.int64(tables[n].shape[0])
        counts = []
        for i, c in enumerate(cases.calls(n)):
            (nf,) = struct.unpack_from("<i", data, off)
            off += 4
            frames = np.frombuffer(data, dtype="<f4", count=nf * 16, offset=off).reshape(nf, 16).copy()
            off += nf * 64
            key = "%s__%d" % (n, i)
            out[key + "__cfg"] = np.asarray(c, dtype=np.float64)
            out[key + "__count"] = np.int64(nf)
            if nf <= cases.FULL_FRAMES:
                out[key + "__frames"] = frames
            else:
                out[key + "__sha256"] = np.frombuffer(cases.frames_sha256(frames).encode(), dtype=np.uint8)
                out[key + "__strided"] = frames[:: cases.FRAME_STRIDE].copy()
            counts.append(nf)
        print(n, tables[n].shape[0], "events", counts, "frames")
    assert off == len(data)
    path = os.path.join(HERE, "tracks_edges_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
