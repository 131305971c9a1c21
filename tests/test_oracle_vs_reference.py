"""Oracle vs the REAL reference on seeded random tracks.

tests/golden/random_golden.npz holds what oracle/_ref/ref_vtm (compiled from the reference sources by oracle/Makefile)
produced for these tracks: sample count, SHA-256 of the float32 output and a strided subset
(tests/golden/make_random_golden.py), so that the comparison runs in every checkout.
"""
import pytest

import golden_cases
import oracle
import tracks


@pytest.mark.parametrize("model,delay,layout,fm", [("0", 1, 0, 0), ("2", 1, 0, 0), ("2:2", 2, 0, 0), ("2:4", 4, 0, 0), ("3", 3, 0, 0), ("4", 1, 1, 0),
                                                    ("1", 1, 0, 1), ("2f:2", 2, 0, 1), ("2f:4", 4, 0, 1), ("4f", 1, 1, 1)])
@pytest.mark.parametrize("seed", [11, 12])
def test_bit_identical_on_random_tracks(model, delay, layout, fm, seed):
    tr = tracks.random_track(90, seed, consonant_heavy=bool(seed & 1))
    out = oracle.synthesize(oracle.male_config(section_delay=delay, layout=layout, float_model=fm), tr)
    golden_cases.check_against_random_golden(out, model, seed)
