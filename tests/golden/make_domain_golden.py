#!/usr/bin/env python3
"""Generates tests/golden/vtm_domain_golden.npz by running the REAL reference on the out-of-range parameter frames of
tests/domain_cases.py: every case in each of the six classes of domain_cases.CLASSES, full samples.

Build-container only: executes oracle/_ref/ref_vtm (compiled in place from the reference's sources by oracle/Makefile
with -O2 -ffp-contract=off).  The .npz holds data only: the reference's samples (one array per class, the cases' vectors
back to back: it compresses a sixth better than an array per vector), and per vector its offset there, the count, the
internal rate, the SHA-256 and the peak.  A bandwidth case needs the class's internal rate before the reference runs: it is taken
from the oracle's design and must be the rate the reference then reports.

    python tests/golden/make_domain_golden.py
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import domain_cases  # noqa: E402
import oracle  # noqa: E402


def main():
    out, manifest = {}, {}
    for cls in domain_cases.CLASSES:
        vectors, offset = [], 0
        model, delay, layout, fm = cls
        fs = float(oracle.derive(oracle.male_config(domain_cases.RATE, delay, layout, float_model=fm)).sample_rate)
        for case in domain_cases.CASES:
            k = domain_cases.key(case, cls)
            ref, info = oracle.ref_synthesize(domain_cases.track_for(case, fs), model, domain_cases.RATE, 250.0)
            assert float(info["fs"]) == fs, (k, info["fs"], fs)
            peak = float(np.abs(ref).max())
            assert np.isfinite(ref).all() and peak > 0.0, k
            manifest[k] = dict(n=int(ref.size), offset=offset, fs=fs, peak=peak, sha256=hashlib.sha256(ref.tobytes()).hexdigest())
            vectors.append(ref)
            offset += int(ref.size)
            print(k, ref.size, peak, manifest[k]["sha256"][:12])
        out[domain_cases.class_key(cls)] = np.concatenate(vectors)
    out["manifest_json"] = np.frombuffer(json.dumps(manifest, sort_keys=True).encode(), dtype=np.uint8)
    np.savez_compressed(os.path.join(HERE, "vtm_domain_golden.npz"), **out)


if __name__ == "__main__":
    main()
