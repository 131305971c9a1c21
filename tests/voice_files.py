"""The voice files of the tests, by name: the five GamaTTS variants of data/voice/english/0_male (tests/golden/voice_*.txt:
vocal tract 17.5 / 15 / 12.5 / 10 / 7.5 cm) and of 5_male, their reference model 5 counterparts (voice5_*.txt), and the
reference's vectors of the latter.  Needs the oracle binding only, not the product: the fixture lists and the scripts
under tests/golden/ import it."""
import functools
import json
import os

import numpy as np

import oracle

# voice id v of the tests' mixed plans is VOICES[v]
VOICES = ["male", "female", "large_child", "small_child", "baby"]


def voice_path(name, model5=False):
    return os.path.join(oracle.GOLDEN_DIR, "voice%s_%s.txt" % ("5" if model5 else "", name))


@functools.lru_cache(maxsize=None)
def golden5v():
    """The reference's vectors of the four 5_male variants besides male (tests/golden/make_voices5_golden.py)."""
    z = np.load(os.path.join(oracle.GOLDEN_DIR, "voices5_golden.npz"), allow_pickle=False)
    data = {k: z[k] for k in z.files}
    data["manifest"] = json.loads(bytes(data.pop("manifest_json")).decode())
    return data
