#!/usr/bin/env python3
"""Generates tests/golden/voice_keys_golden.npz by running the REAL reference on the voice-key sets of
tests/voice_key_cases.py: every set under the model string and output rate of every cell ("0", "1", "2:2", "2f:3", "4",
"4f"), both model 5 sets under "5" and "5f" at 48 kHz, all on the table's one 24-frame track.

Build-container only: executes oracle/_ref/ref_vtm (compiled in place from the reference sources by oracle/Makefile with
-O2 -ffp-contract=off).  The .npz holds data only: per run the sample count, internal steps and rate, the SHA-256 of the
float32 output and every DIGEST_STRIDE-th sample.

    python tests/golden/make_voice_keys_golden.py
"""
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import golden_cases  # noqa: E402
import oracle  # noqa: E402
import voice_key_cases as cases  # noqa: E402


def main():
    if oracle.ref_binary() is None:
        sys.exit("oracle/_ref/ref_vtm is not built (build() makes it where the reference sources are)")
    tr = cases.track()
    out, manifest = {}, {}
    for key, overrides, model5, model, rate in cases.reference_runs():
        keys = oracle.read_config_file(oracle.VOICE5_MALE if model5 else oracle.VOICE_MALE)
        keys.update({k: repr(v) for k, v in overrides.items()})
        with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
            for k, v in keys.items():
                f.write("%s = %s\n" % (k, v))
            cfg_path = f.name
        try:
            ref, info = oracle.ref_synthesize(tr, model, rate, cases.CRATE, config=cfg_path)
        finally:
            os.unlink(cfg_path)
        assert np.isfinite(ref).all() and ref.size, key
        manifest[key] = dict(n=int(ref.size), steps=int(info["steps"]), fs=float(info["fs"]), model=model, rate=rate,
                             maxabs=float(np.abs(ref).max()), sha256=hashlib.sha256(ref.tobytes()).hexdigest())
        out[key + "__strided"] = ref[:: golden_cases.DIGEST_STRIDE].copy()
        print(key, ref.size, manifest[key]["steps"], manifest[key]["fs"], manifest[key]["sha256"][:12])
    out["manifest_json"] = np.frombuffer(json.dumps(manifest, sort_keys=True).encode(), dtype=np.uint8)
    np.savez_compressed(os.path.join(HERE, "voice_keys_golden.npz"), **out)
    print("wrote", os.path.join(HERE, "voice_keys_golden.npz"))


if __name__ == "__main__":
    main()
