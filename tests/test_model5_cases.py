"""Pins the case table of reference model 5 (model5_cases.py) against its vector files: a case without a vector, a vector
without a case or an array no case stores fails here, in milliseconds.  No GPU needed."""
import numpy as np
import pytest

import model5_cases as cases


@pytest.mark.parametrize("fixture", list(cases.CASES))
def test_the_file_holds_the_tables_cases_and_nothing_else(fixture):
    data = cases.load(fixture)
    assert all(c["fixture"] == fixture for c in cases.CASES[fixture])
    assert sorted(data["manifest"]) == sorted(c["name"] for c in cases.CASES[fixture])
    keys = [key for c in cases.CASES[fixture] for _, key in cases.stored(c, np.zeros(0, np.float32))]
    assert sorted(keys) == sorted(k for k in data if k != "manifest")
