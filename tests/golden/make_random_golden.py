#!/usr/bin/env python3
"""Generates tests/golden/random_golden.npz by running the REAL reference on the seeded random tracks of
tests/test_oracle_vs_reference.py and tests/test_oracle5_vs_golden.py::test_oracle5_matches_reference_binary_on_fresh_tracks.

Build-container only: executes oracle/_ref/ref_vtm (compiled in place from the reference sources by oracle/Makefile with
-O2 -ffp-contract=off).  The .npz holds data only: per case the sample count, internal steps and rate, the SHA-256 of
the float32 output and every DIGEST_STRIDE-th sample.

    python tests/golden/make_random_golden.py
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import golden_cases  # noqa: E402
import oracle  # noqa: E402
import tracks  # noqa: E402

# (reference model, seed, frames, consonant_heavy, output rate, voice)
CASES = [(m, s, 90, bool(s & 1), 44100, oracle.VOICE_MALE)
         for m in ("0", "2", "2:2", "2:4", "3", "4", "1", "2f:2", "2f:4", "4f") for s in (11, 12)]
CASES += [(m, s, 60, s % 2 == 0, 48000, oracle.VOICE5_MALE) for m in ("5", "5f") for s in (31, 32)]


def key(model, seed):
    return "m%s_s%d" % (model.replace(":", "d"), seed)


def main():
    out, manifest = {}, {}
    for model, seed, frames, heavy, rate, voice in CASES:
        tr = tracks.random_track(frames, seed, consonant_heavy=heavy)
        ref, info = oracle.ref_synthesize(tr, model, rate, 250, config=voice)
        k = key(model, seed)
        manifest[k] = dict(n=int(ref.size), steps=int(info["steps"]), fs=float(info["fs"]),
                           sha256=hashlib.sha256(ref.tobytes()).hexdigest())
        out[k + "__strided"] = ref[:: golden_cases.DIGEST_STRIDE].copy()
        print(k, ref.size, manifest[k]["sha256"][:12])
    out["manifest_json"] = np.frombuffer(json.dumps(manifest, sort_keys=True).encode(), dtype=np.uint8)
    np.savez_compressed(os.path.join(HERE, "random_golden.npz"), **out)


if __name__ == "__main__":
    main()
