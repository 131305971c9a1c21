"""Track generation at the device kernel's edges, without a GPU: the oracle against the reference's frames for the lists of
tracks_edges_cases.py (tests/golden/tracks_edges_golden.npz), the product's frame counter on them, the generators those
lists come from, and the alignment check of gvtm_generate_tracks_device."""
import os

import numpy as np
import pytest

from gama_tts_amd import capi
import event_lists
import oracle
import tracks_edges_cases as cases
from track_cases import product_config

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def edges():
    z = np.load(os.path.join(HERE, "golden", "tracks_edges_golden.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def tables(golden_tracks):
    return {n: cases.table(n, golden_tracks) for n in cases.LISTS}


def test_fixture_covers_every_list_and_the_lists_are_what_it_was_made_from(edges, tables):
    assert {k.split("__")[0] for k in edges} == set(cases.LISTS)
    for n, t in tables.items():
        assert int(edges[n + "__events"]) == t.shape[0], n
        assert bytes(edges[n + "__table_sha256"]).decode() == cases.table_sha256(t), n  # a generator drifted
        for i, c in enumerate(cases.calls(n)):
            assert np.array_equal(edges["%s__%d__cfg" % (n, i)], c), (n, i)


@pytest.mark.parametrize("name", list(cases.LISTS))
def test_oracle_matches_reference_at_the_edges(name, edges, tables):
    """Every call of the list, the drift generator running on from call to call as in the reference's EventList: the
    reference's frames bit for bit (NaN bits included: both run on the same CPU)."""
    state = oracle.FRESH_DRIFT
    for i, c in enumerate(cases.calls(name)):
        frames, state = oracle.tracks_generate(oracle.track_config(c), tables[name], state)
        msg = cases.check_frames(edges, name, i, frames)
        assert msg is None, msg


@pytest.mark.parametrize("name", list(cases.LISTS))
def test_frame_count_matches_reference_at_the_edges(name, edges, tables):
    ev = capi.events_from_table(tables[name])
    for i, c in enumerate(cases.calls(name)):
        assert capi.tracks_frame_count(product_config(c), ev) == int(edges["%s__%d__count" % (name, i)]), (name, i)


def test_edge_lists_have_the_shapes_they_are_named_for(tables):
    """What the GPU tests rely on: the boundary layouts, the far gaps, the times."""
    def gaps(t, c):
        rows = np.flatnonzero(~np.isinf(t[:, 6 + c]))
        return rows, np.diff(rows)
    for n in (239, 240, 241, 242):
        t = tables["b%d" % n]
        assert t.shape[0] == n
        assert gaps(t, event_lists.FAR_PARAM)[0].tolist() == [0, 1, n - 1]
        assert gaps(t, event_lists.FAR_SPECIAL)[0].tolist() == [0, n - 1]
        assert gaps(t, event_lists.FIRST_SPECIAL)[0].tolist() == [0]
        assert gaps(t, event_lists.NEVER_SPECIAL)[0].size == 0
        assert (t[:, 0] % 4 == 0).all()
    assert max(gaps(tables["far1000"], 16 + 7)[1]) > 255 and max(gaps(tables["far1000"], 12)[1]) > 255
    assert 2000 <= tables["joined2600"].shape[0] <= 3000 and (np.diff(tables["joined2600"][:, 0]) > 0).all()
    for cp in (2, 3, 4):
        t = tables["offgrid_cp%d" % cp][:, 0]
        assert (t[1:] % cp != 0).all() and (np.diff(t) < cp).any()
    for cp in (1, 2, 3, 4):
        assert (np.diff(tables["subperiod_cp%d" % cp][:, 0]) == 0).any()
    assert np.isinf(tables["unset_first"][0, 6 + 3]) and not np.isinf(tables["unset_first"][1:, 6 + 3]).all()
    assert not tables["interp_none"][:, 1].any()
    assert tables["interp_last"][:, 1].tolist() == [0.0] * 79 + [1.0]


def test_generator_options():
    t = event_lists.random_event_table(3, n_events=200, control_period=4, max_gap_periods=2, min_gap_ms=0,
                                       special_rate=[0.0] + [0.5] * 15, force_set={16: [7], 4: [0, 9]}, force_unset={5: [0, 1]})
    d = np.diff(t[:, 0])
    assert d.min() == 0 and d.max() <= 8 and (d % 4 != 0).any()
    assert np.flatnonzero(~np.isinf(t[:, 22])).tolist() == [7]
    assert np.isinf(t[:2, 6 + 5]).all() and not np.isinf(t[[0, 9], 6 + 4]).any()
    assert event_lists.boundary_table(2).shape == (2, 38) and event_lists.boundary_table(0).shape == (0, 38)


def test_generate_tracks_device_rejects_unaligned_params():
    """Frames leave the kernel as 16-byte stores: a d_params that is not 16-byte aligned is refused before anything touches
    a device (the pointers here are never dereferenced)."""
    cfg = product_config(cases.cfg())
    with pytest.raises(capi.GvtmError) as ei:
        capi.generate_tracks_device(cfg, 0x2000, 0x3000, 1, 8, 0x1004)
    assert ei.value.status == 1  # GVTM_ERR_INVALID_ARGUMENT
    assert "aligned" in str(ei.value)
    for bad in (0x1001, 0x1008, 0x100C):
        with pytest.raises(capi.GvtmError) as ei:
            capi.generate_tracks_device(cfg, 0x2000, 0x3000, 3, 8, bad)
        assert ei.value.status == 1
