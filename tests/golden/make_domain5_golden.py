#!/usr/bin/env python3
"""Generates tests/golden/vtm5_domain_golden.npz by running the REAL reference's VocalTractModel5<double,1> (model "5")
and VocalTractModel5<float,1> (model "5f") on the out-of-range parameter frames of tests/domain5_cases.py: every case with
a reference, in each configuration it names (the male, female and baby voice files; 5_male with one override, written to
a temporary file), full samples.

Build-container only: executes oracle/_ref/ref_vtm (compiled in place from the reference's sources by oracle/Makefile
with -O2 -ffp-contract=off).  The .npz holds data only: the reference's samples (one array per class and configuration,
the cases' vectors back to back), and per vector its offset there, the count, the internal rate, the SHA-256 and the
peak.  The product-rule cases (reference=False: sections outside S1..S30, where the reference indexes out of bounds) are
never run; the script asserts that it skipped them.

    python tests/golden/make_domain5_golden.py
"""
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import domain5_cases as cases  # noqa: E402
import oracle  # noqa: E402


def main():
    if oracle.ref_binary() is None:
        sys.exit("oracle/_ref/ref_vtm is not built (build() makes it where the reference sources are)")
    out, manifest, made = {}, {}, set()
    for cls in cases.CLASSES:
        for config in cases.CONFIGS:
            with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
                for k, v in cases.config_keys(config).items():
                    f.write("%s = %s\n" % (k, v))
                cfg_path = f.name
            vectors, offset = [], 0
            try:
                for case in cases.cases_of(config):
                    assert case["reference"]
                    k = cases.key(case, config, cls)
                    ref, info = oracle.ref_synthesize(cases.track_for(case), cls[0], cases.RATE, cases.CRATE, config=cfg_path)
                    peak = float(np.abs(ref).max())
                    assert np.isfinite(ref).all() and peak > 0.0, k
                    manifest[k] = dict(n=int(ref.size), offset=offset, fs=float(info["fs"]), peak=peak,
                                       sha256=hashlib.sha256(ref.tobytes()).hexdigest())
                    vectors.append(ref)
                    offset += int(ref.size)
                    made.add(case["name"])
                    print(k, ref.size, manifest[k]["fs"], peak, manifest[k]["sha256"][:12])
            finally:
                os.unlink(cfg_path)
            out[cases.block_key(config, cls)] = np.concatenate(vectors)
    skipped = [c["name"] for c in cases.CASES if c["name"] not in made]
    assert skipped == [c["name"] for c in cases.PRODUCT_CASES] and len(skipped) == 9, skipped
    assert list(manifest) == [cases.key(*v) for v in cases.vector_keys()]
    out["manifest_json"] = np.frombuffer(json.dumps(manifest, sort_keys=True).encode(), dtype=np.uint8)
    np.savez_compressed(cases.GOLDEN, **out)
    print("%d vectors, %d bytes" % (len(manifest), os.path.getsize(cases.GOLDEN)))


if __name__ == "__main__":
    main()
