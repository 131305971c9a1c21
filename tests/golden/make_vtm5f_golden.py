#!/usr/bin/env python3
"""Generates tests/golden/vtm5f_golden.npz by running the REAL reference's VocalTractModel5<float,1> (model "5f").

Build-container only: executes oracle/_ref/ref_vtm (compiled from the reference sources by oracle/Makefile with -O2
-ffp-contract=off).  The .npz holds data only: reference output samples (full, or every DIGEST_STRIDE-th with the
SHA-256 of all), counts, steps, the internal rate.  Input frames are the recipes of tests/golden5f_cases.py.

    python tests/golden/make_vtm5f_golden.py
"""
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import golden5f_cases  # noqa: E402
import oracle  # noqa: E402


def main():
    out, manifest = {}, {}
    for case in golden5f_cases.CASES:
        name = case["name"]
        tr = golden5f_cases.track_for(case)
        with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
            for k, v in golden5f_cases.config_dict(case).items():
                f.write("%s = %s\n" % (k, v))
            cfg_path = f.name
        try:
            ref, info = oracle.ref_synthesize(tr, case["model"], case["rate"], case["crate"], config=cfg_path)
        finally:
            os.unlink(cfg_path)
        manifest[name] = dict(n=int(ref.size), steps=int(info["steps"]), fs=float(info["fs"]), frames=int(tr.shape[0]),
                              sum=float(ref.astype(np.float64).sum()), maxabs=float(np.abs(ref).max()) if ref.size else 0.0,
                              sha256=hashlib.sha256(ref.tobytes()).hexdigest())
        if case["store"] == "full":
            out[name + "__out"] = ref
        else:
            out[name + "__strided"] = ref[:: golden5f_cases.DIGEST_STRIDE].copy()
        print(name, ref.size, manifest[name]["sha256"][:12])
    out["manifest_json"] = np.frombuffer(json.dumps(manifest, sort_keys=True).encode(), dtype=np.uint8)
    np.savez_compressed(golden5f_cases.GOLDEN, **out)


if __name__ == "__main__":
    main()
