#!/usr/bin/env python3
"""Generates the vector files of reference model 5 (tests/golden/{vtm5,vtm5f,voices5,voices5f}_golden.npz) by running the
REAL reference's VocalTractModel5<double,1> (model "5") and VocalTractModel5<float,1> (model "5f").

Build-container only: executes oracle/_ref/ref_vtm (compiled from the reference sources by oracle/Makefile with -O2
-ffp-contract=off).  An .npz holds data only: reference output samples (full, or every DIGEST_STRIDE-th with the SHA-256
of all, and the last OVERRUN_TAIL of a "tail" case), counts, steps, the internal rate.  Input frames are the recipes of
tests/model5_cases.py (the "hello" frames are the ones stored in vtm_golden.npz).

Every "tail" case must sit on a flush overrun of the converter: the reference itself has to give more samples for its
length than for one frame more, or the script stops.

    python tests/golden/make_model5_golden.py vtm5|vtm5f|voices5|voices5f|all [--out DIR]
"""
import argparse
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import model5_cases as cases  # noqa: E402
import oracle  # noqa: E402

WITH_FRAMES = ("vtm5f", "voices5f")  # the fixtures whose manifest has the frame count


def reference(case, tr, cfg_path):
    return oracle.ref_synthesize(tr, case["model"], case["rate"], case["crate"], config=cfg_path)


def make(fixture, out_dir, hello):
    out, manifest = {}, {}
    for case in cases.CASES[fixture]:
        name = case["name"]
        tr = cases.track_for(case, hello)
        with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
            for k, v in cases.config_keys(case).items():
                f.write("%s = %s\n" % (k, v))
            cfg_path = f.name
        try:
            ref, info = reference(case, tr, cfg_path)
            if case["store"] == "tail":
                more, _ = reference(case, np.concatenate([tr, tr[-1:]]), cfg_path)
                assert ref.size > more.size, "%s: %d frames are no flush overrun (%d samples, %d for one frame more)" % (
                    name, tr.shape[0], ref.size, more.size)
        finally:
            os.unlink(cfg_path)
        manifest[name] = dict(n=int(ref.size), steps=int(info["steps"]), fs=float(info["fs"]),
                              sum=float(ref.astype(np.float64).sum()), maxabs=float(np.abs(ref).max()) if ref.size else 0.0,
                              sha256=hashlib.sha256(ref.tobytes()).hexdigest())
        if fixture in WITH_FRAMES:
            manifest[name]["frames"] = int(tr.shape[0])
        for part, key in cases.stored(case, ref):
            out[key] = part.copy()
        print(name, ref.size, manifest[name]["fs"], manifest[name]["sha256"][:12])
    out["manifest_json"] = np.frombuffer(json.dumps(manifest, sort_keys=True).encode(), dtype=np.uint8)
    np.savez_compressed(os.path.join(out_dir, os.path.basename(cases.golden_path(fixture))), **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("fixture", choices=list(cases.CASES) + ["all"])
    ap.add_argument("--out", default=HERE, help="directory to write to (default: tests/golden)")
    args = ap.parse_args()
    if oracle.ref_binary() is None:
        sys.exit("oracle/_ref/ref_vtm is not built (build() makes it where the reference sources are)")
    hello = {"hello_params": np.load(os.path.join(HERE, "vtm_golden.npz"), allow_pickle=False)["hello_params"]}
    os.makedirs(args.out, exist_ok=True)
    for fixture in cases.CASES if args.fixture == "all" else [args.fixture]:
        make(fixture, args.out, hello)


if __name__ == "__main__":
    main()
