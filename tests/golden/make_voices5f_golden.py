#!/usr/bin/env python3
"""Generates tests/golden/voices5f_golden.npz by running the REAL reference's VocalTractModel5<float,1> (model "5f") with
the four 5_male variants besides male (tests/golden/voice5_{female,large_child,small_child,baby}.txt), and both classes
(models "5f" and "5") at the limits of the sample-rate converter.

Build-container only: executes oracle/_ref/ref_vtm (compiled in place from the reference sources by oracle/Makefile with
-O2 -ffp-contract=off).  The .npz holds data only: reference output samples (full, or every DIGEST_STRIDE-th with the
SHA-256 of all, and the last OVERRUN_TAIL of an overrun case), counts, steps, the internal rate.  Input frames are the
recipes of tests/golden5f_voices_cases.py (the "hello" frames are the ones stored in vtm_golden.npz).

Every <voice>_ovr_5f case must sit on a flush overrun of the float converter: the reference itself has to give more
samples for its length than for one frame more, or the script stops.

    python tests/golden/make_voices5f_golden.py
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import golden5f_voices_cases as cases  # noqa: E402
import oracle  # noqa: E402
import voice_files  # noqa: E402


def main():
    if oracle.ref_binary() is None:
        sys.exit("oracle/_ref/ref_vtm is not built (build() makes it where the reference sources are)")
    hello = {"hello_params": np.load(os.path.join(HERE, "vtm_golden.npz"), allow_pickle=False)["hello_params"]}
    out, manifest = {}, {}
    for case in cases.CASES:
        name = case["name"]
        tr = cases.track_for(case, hello)
        config = voice_files.voice_path(case["voice"], model5=True)
        ref, info = oracle.ref_synthesize(tr, case["model"], case["rate"], case["crate"], config=config)
        if case["store"] == "tail":
            longer = np.concatenate([tr, tr[-1:]])
            more, _ = oracle.ref_synthesize(longer, case["model"], case["rate"], case["crate"], config=config)
            assert ref.size > more.size, "%s: %d frames are no flush overrun (%d samples, %d for one frame more)" % (
                name, tr.shape[0], ref.size, more.size)
        manifest[name] = dict(n=int(ref.size), steps=int(info["steps"]), fs=float(info["fs"]), frames=int(tr.shape[0]),
                              sum=float(ref.astype(np.float64).sum()), maxabs=float(np.abs(ref).max()) if ref.size else 0.0,
                              sha256=hashlib.sha256(ref.tobytes()).hexdigest())
        if case["store"] == "full":
            out[name + "__out"] = ref
        else:
            out[name + "__strided"] = ref[:: cases.DIGEST_STRIDE].copy()
        if case["store"] == "tail":
            out[name + "__tail"] = ref[-cases.OVERRUN_TAIL:].copy()
        print(name, ref.size, manifest[name]["fs"], manifest[name]["sha256"][:12])
    out["manifest_json"] = np.frombuffer(json.dumps(manifest, sort_keys=True).encode(), dtype=np.uint8)
    np.savez_compressed(cases.GOLDEN, **out)


if __name__ == "__main__":
    main()
