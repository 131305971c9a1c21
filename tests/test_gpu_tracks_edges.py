"""Device track generation (gvtm_generate_tracks_device, vtm_tracks.hip) at the edges of its design, bit for bit against
the tracks oracle and, where the lists are those of tests/golden/tracks_edges_golden.npz, against the reference's frames:
lists on either side of the LDS table (kTableEvents = 240) in one wavefront (utterances 2k and 2k + 1), columns whose next
set event lies far away, lists of up to 6,000 events, the 32-frame ring and its flushes against max_frames, times off the
control-period grid and several events inside one period at control periods 1 to 4, every flag combination with drift
generators that ran before, a batch of 4,097, the events entry, and the same walk as the voices and the chunks entries
compile it (per-utterance constants; one list per utterance as one chunk).

Frames are compared as bits (view(uint32)), drift states as bits (view(int64)).  One exception: where the oracle's frame is
NaN the device's must be NaN, of any sign and payload (0 / 0 and inf - inf give the x86 default NaN, sign bit set, on the
host; the device's default NaN may differ)."""
import os

import numpy as np
import pytest

import gama_tts_amd as g
from gama_tts_amd import capi
import event_lists
import oracle
import tracks_edges_cases as cases
from chunk_cases import generate_tracks_chunks
from device_io import current_stream, events_chain_and_entry, events_on_device, to_device
from track_cases import product_config
from voice_cases import configs, male_plan
from voice_files import VOICES

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL = 0x7FC0DEAD  # a quiet NaN that marks frames the kernel must not write
GUARD_FRAMES = 64


@pytest.fixture(scope="module")
def edges():
    z = np.load(os.path.join(HERE, "golden", "tracks_edges_golden.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def tables(golden_tracks):
    t = {n: cases.table(n, golden_tracks) for n in cases.LISTS}
    for n in (1000, 3000, 6000):
        t["joined%d" % n] = event_lists.joined_captured(golden_tracks, n)
    t["synth3000"] = event_lists.random_event_table(3000, n_events=3000)
    t["far6000"] = cases._far_gaps(6000)
    for n in (0, 1, 2):
        t["e%d" % n] = event_lists.boundary_table(n, seed=50 + n)
    for c in (1, 31, 32, 33, 63, 64, 65, 100):
        t["frames%d" % c] = _list_with_frames(c)
    return t


def _list_with_frames(count, cp=4):
    """A list that yields exactly `count` frames at control period cp: times on the grid, the last at count periods."""
    n = min(count, 6) + 1
    t = event_lists.random_event_table(4000 + count, n_events=n, control_period=cp)
    steps = np.linspace(0, count, n).round().astype(np.int64)
    steps[-1] = count
    t[:, 0] = cp * steps
    return t


def _states(n, seed):
    """n drift-generator states that have run before (seed in (0.1, 0.9), filter memory of the size drift leaves)."""
    rng = np.random.default_rng(seed)
    s = np.zeros((n, 5))
    s[:, 0] = rng.uniform(0.1, 0.9, n)
    s[:, 1:] = rng.uniform(-4.0, 4.0, (n, 4))
    return s


NAN_BITS = set()  # device bit patterns seen where the oracle has NaN


def _assert_frames(got, want, what):
    """got: the device's frames, want: the oracle's or the reference's; bit for bit but for the NaN rule above."""
    assert got.shape == want.shape, what
    wn = np.isnan(want)
    gb, wb = got.view(np.uint32), want.view(np.uint32)
    if not np.array_equal(np.isnan(got), wn):
        bad = np.argwhere(np.isnan(got) != wn)[0]
        raise AssertionError("%s: NaN at %s (device %#x, oracle %#x)" % (what, bad.tolist(), gb[tuple(bad)], wb[tuple(bad)]))
    diff = (gb != wb) & ~wn
    if diff.any():
        bad = np.argwhere(diff)
        raise AssertionError("%s: %d values differ, first at %s (device %r, oracle %r)"
                             % (what, bad.shape[0], bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))
    NAN_BITS.update(np.unique(gb[wn]).tolist())


def _check_fixture(edges, name, call, frames):
    """frames: the device's for call `call` of list `name` of the fixture (the reference's frames; whole, or every
    FRAME_STRIDE-th frame plus the SHA-256 of all, which only NaN-free frames can match bit for bit)."""
    key = "%s__%d" % (name, call)
    assert frames.shape[0] == int(edges[key + "__count"]), key
    if key + "__frames" in edges:
        _assert_frames(frames, edges[key + "__frames"], key)
    else:
        _assert_frames(frames[:: cases.FRAME_STRIDE], edges[key + "__strided"], key)
        if not np.isnan(frames).any():
            assert cases.frames_sha256(frames) == bytes(edges[key + "__sha256"]).decode(), key


def _launch(cfg, tabs, max_frames, drift_in):
    """gvtm_generate_tracks_device on a buffer filled with SENTINEL (GUARD_FRAMES more frames behind the last row) ->
    (params [B][max_frames][16], guard, counts, drift out), all on the host."""
    import torch
    d_events, d_offsets = events_on_device(tabs)
    dev = d_events.device
    b = len(tabs)
    buf = torch.full(((b * max_frames + GUARD_FRAMES) * 16,), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
    counts = torch.full((b,), -7, dtype=torch.int32, device=dev)
    drift = torch.from_numpy(np.ascontiguousarray(drift_in, dtype=np.float64)).to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    capi.generate_tracks_device(product_config(cfg), d_events, d_offsets, b, max_frames, buf, counts, drift, stream)
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    params = out[: b * max_frames * 16].reshape(b, max_frames, 16)
    return params, out[b * max_frames * 16:], counts.cpu().numpy(), drift.cpu().numpy()


def _check_rows(cfg, tabs, max_frames, drift_in, got, what, oracle_cache=None):
    """Every row against the oracle: count in full, frames [0, min(count, max_frames)) bit for bit, SENTINEL behind them,
    drift state bit for bit (rows of fewer than two events: the one they came in with).  Returns the oracle's frames."""
    params, guard, counts, drift = got
    assert (guard.view(np.uint32) == SENTINEL).all(), "%s: written past the last row" % what
    want_all = []
    for b, t in enumerate(tabs):
        key = (id(t), tuple(drift_in[b]))
        if oracle_cache is not None and key in oracle_cache:
            frames, state = oracle_cache[key]
        else:
            frames, state = oracle.tracks_generate(oracle.track_config(cfg), t, tuple(drift_in[b]))
            if oracle_cache is not None:
                oracle_cache[key] = (frames, state)
        want_all.append(frames)
        assert counts[b] == frames.shape[0], (what, b, counts[b], frames.shape[0])
        m = min(frames.shape[0], max_frames)
        _assert_frames(params[b, :m], frames[:m], "%s row %d (%d events)" % (what, b, t.shape[0]))
        assert (params[b, m:].view(np.uint32) == SENTINEL).all(), (what, b, "frame written past min(count, max_frames)")
        assert np.array_equal(drift[b].view(np.int64), np.asarray(state, dtype=np.float64).view(np.int64)), (what, b)
        if t.shape[0] < 2:
            assert np.array_equal(drift[b].view(np.int64), np.asarray(drift_in[b], dtype=np.float64).view(np.int64)), (what, b)
    return want_all


def _chain(names, tables, calls, drift0, max_frames=None):
    """The calls one after the other on one batch, each call's drift states the next one's; yields (call, cfg, got, drift_in)."""
    tabs = [tables[n] for n in names]
    drift = np.array(drift0, dtype=np.float64)
    for i, cfg in enumerate(calls):
        mf = max_frames or max(1, max(capi.tracks_frame_count(product_config(cfg), capi.events_from_table(t)) for t in tabs))
        got = _launch(cfg, tabs, mf, drift)
        yield i, cfg, tabs, mf, got, drift
        drift = got[3].copy()


@pytest.mark.parametrize("name", list(cases.LISTS))
def test_device_matches_reference_at_the_edges(name, tables, edges):
    """Each list of the fixture as utterance 1 of a wavefront whose utterance 0 is a 2-event list, the fixture's calls chained
    from a fresh drift generator: the reference's frames, and the oracle's drift states."""
    names = ["e2", name, "e0"]
    drift0 = np.tile(np.array(oracle.FRESH_DRIFT), (3, 1))
    for i, cfg, tabs, mf, got, din in _chain(names, tables, cases.calls(name), drift0):
        _check_rows(cfg, tabs, mf, din, got, "%s call %d" % (name, i))
        _check_fixture(edges, name, i, got[0][1, : got[2][1]])


@pytest.mark.parametrize("flags", [(1, 1, 1, 1), (0, 1, 1, 0), (1, 0, 0, 1), (1, 1, 0, 0)])
def test_table_boundary_pairs_in_one_wavefront(flags, tables, edges):
    """Utterances (2k, 2k + 1): (240, 241), (239, 2), (241, 0), (242, 240) events -- a tabled and an untabled list, a
    tabled list next to a short one, an untabled one next to an empty row; two chained calls, the short and empty rows
    with generators that ran before."""
    names = ["b240", "b241", "b239", "e2", "b241", "e0", "b242", "b240"]
    drift0 = np.tile(np.array(oracle.FRESH_DRIFT), (len(names), 1))
    drift0[[3, 5]] = _states(2, 11)
    cfg = cases.cfg(4, *flags)
    for i, cfg, tabs, mf, got, din in _chain(names, tables, [cfg, cfg], drift0):
        _check_rows(cfg, tabs, mf, din, got, "pairs %s call %d" % (flags, i))
    # the same batch with the fixture's calls: the boundary rows start from fresh generators, as the fixture's chains do
    for i, cfg, tabs, mf, got, din in _chain(names, tables, cases.calls("b240"), drift0):
        _check_rows(cfg, tabs, mf, din, got, "pairs fixture call %d" % i)
        for b, n in enumerate(names):
            if n.startswith("b"):
                _check_fixture(edges, n, i, got[0][b, : got[2][b]])


def test_long_lists_next_to_short_ones(tables, edges):
    """1,000 to 6,000 events, captured speech joined and synthetic (special columns with gaps of thousands of events), an
    odd batch whose short rows share wavefronts with long ones."""
    names = ["far1000", "e2", "joined3000", "e2", "joined6000", "synth3000", "e2", "joined2600", "far6000", "joined1000", "e1"]
    drift0 = np.tile(np.array(oracle.FRESH_DRIFT), (len(names), 1))
    drift0[[1, 3, 6, 10]] = _states(4, 12)
    calls = [cases.cfg(), cases.cfg(4, 1, 1, 1, 0)]
    for i, cfg, tabs, mf, got, din in _chain(names, tables, calls, drift0):
        _check_rows(cfg, tabs, mf, din, got, "long call %d" % i)
        assert mf > 25000
        _check_fixture(edges, "joined2600", i, got[0][7, : got[2][7]])
        if i == 0:
            _check_fixture(edges, "far1000", 0, got[0][0, : got[2][0]])


@pytest.mark.parametrize("max_frames", [31, 32, 33, 65, 70])
def test_ring_flushes_and_truncation(max_frames, tables):
    """Lists of 1, 31, 32, 33, 63, 64, 65 and 100 frames, each followed by a row of 0 or 1 events, on a buffer of sentinel
    NaNs: frame i of a row is written iff i < min(count, max_frames) (a write past max_frames would land in the following
    row, which must stay untouched), counts in full, rows of fewer than two events keep their drift state and count 0."""
    longs = ["frames%d" % c for c in (1, 31, 32, 33, 63, 64, 65, 100)]
    names = []
    for k, n in enumerate(longs):
        names += [n, "e0" if k % 2 else "e1"]
    cfg = cases.cfg()
    for n in longs:
        assert capi.tracks_frame_count(product_config(cfg), capi.events_from_table(tables[n])) == int(n[6:])
    drift0 = _states(len(names), 13)
    got = _launch(cfg, [tables[n] for n in names], max_frames, drift0)
    _check_rows(cfg, [tables[n] for n in names], max_frames, drift0, got, "ring max_frames=%d" % max_frames)
    for b in range(1, len(names), 2):
        assert got[2][b] == 0 and (got[0][b].view(np.uint32) == SENTINEL).all()
    # and the same lists as the second row of their wavefront
    got = _launch(cfg, [tables[n] for n in names[1:]], max_frames, drift0[1:])
    _check_rows(cfg, [tables[n] for n in names[1:]], max_frames, drift0[1:], got, "ring shifted max_frames=%d" % max_frames)


@pytest.mark.parametrize("cp", [1, 2, 3, 4])
def test_timing_off_grid_and_inside_one_period(cp, tables, edges):
    """Times off the control-period grid, several events inside one period (deltas over 0 and negative times: inf and NaN
    frames), control periods 1 to 4: the reference's frames with fresh generators, the oracle's with generators that ran."""
    names = ["offgrid_cp%d" % cp, "subperiod_cp%d" % cp, "subperiod_cp%d" % cp, "offgrid_cp%d" % cp, "e1"]
    drift0 = np.tile(np.array(oracle.FRESH_DRIFT), (len(names), 1))
    drift0[2:] = _states(3, 14)
    for i, cfg, tabs, mf, got, din in _chain(names, tables, cases.calls(names[0]), drift0):
        _check_rows(cfg, tabs, mf, din, got, "cp %d call %d" % (cp, i))
        for b in (0, 1):
            if cases.calls(names[b])[i].tolist() == cfg.tolist():
                _check_fixture(edges, names[b], i, got[0][b, : got[2][b]])
    print("device NaN bits where the oracle has NaN (cp %d): %s" % (cp, sorted("%#010x" % v for v in NAN_BITS)))


@pytest.mark.parametrize("flags", cases.FLAGS16, ids=["m%di%dd%ds%d" % f for f in cases.FLAGS16])
def test_every_flag_combination_with_generators_that_ran(flags, tables):
    names = ["flags16", "interp_none", "interp_last", "unset_first", "b240", "joined1000", "e1"]
    drift0 = _states(len(names), 15)
    cfg = cases.cfg(4, *flags)
    for i, cfg, tabs, mf, got, din in _chain(names, tables, [cfg, cfg], drift0):
        _check_rows(cfg, tabs, mf, din, got, "flags %s call %d" % (flags, i))


def test_batch_of_4097(tables):
    """4,097 rows drawn from every list above (control period 4), three drift states per list, cut at 600 frames: every
    row against the oracle."""
    pool = ["b239", "b240", "b241", "b242", "e0", "e1", "e2", "offgrid_cp4", "subperiod_cp4", "unset_first", "interp_none",
            "interp_last", "flags16", "far1000", "joined1000", "joined2600", "synth3000"] + ["frames%d" % c for c in (1, 31, 32, 33, 63, 64, 65, 100)]
    rng = np.random.default_rng(4097)
    pick = rng.integers(0, len(pool), 4097)
    states = _states(3, 16)
    drift0 = states[rng.integers(0, 3, 4097)]
    tabs = [tables[pool[k]] for k in pick]
    cfg = cases.cfg()
    got = _launch(cfg, tabs, 600, drift0)
    _check_rows(cfg, tabs, 600, drift0, got, "batch 4097", oracle_cache={})


def test_events_entry_at_the_edges(tables):
    """gvtm_synthesize_events_device on the boundary pairs and a 3,000-event list: the two-call chain bit for bit; the long
    utterance in float against the oracle of the oracle (macro intonation off: the pitch stays inside the model's range)."""
    import torch
    names = ["b240", "b241", "b239", "e2", "b241", "e0", "b242", "b240", "joined3000"]
    tabs = [tables[n] for n in names]
    cfgv = cases.cfg(4, 0, 1, 1, 1)
    tc = product_config(cfgv)
    frames_of = [capi.tracks_frame_count(tc, capi.events_from_table(t)) for t in tabs]
    max_frames = max(frames_of)
    batch = len(tabs)
    drift0 = _states(batch, 17)
    plan = male_plan(precision=capi.PRECISION_F32)
    stride = plan.output_capacity(max_frames)
    chain, entry, d_params = events_chain_and_entry(plan, tc, tabs, max_frames, stride, drift0)
    a1, f1, n1, m1, dr1 = chain
    a2, f2, n2, m2, dr2 = entry
    assert f2.cpu().tolist() == frames_of
    assert torch.equal(f1, f2) and torch.equal(n1, n2)
    assert torch.equal(dr1.view(torch.int64), dr2.view(torch.int64))
    ok = torch.isfinite(a1).all(dim=1) & torch.isfinite(m1)
    assert bool(ok[-1]) and int(ok.sum().item()) >= 4
    assert torch.equal(m1[ok].view(torch.int32), m2[ok].view(torch.int32))
    assert torch.equal(a1[ok].view(torch.int32), a2[ok].view(torch.int32))
    # the frames against the oracle, then one utterance through the float oracle: the 3,000-event list (the reference's own
    # rules set its parameters, inside the model's ranges; the random boundary lists add special offsets that can leave them)
    params = d_params.cpu().numpy()
    for b, t in enumerate(tabs):
        want, _ = oracle.tracks_generate(oracle.track_config(cfgv), t, tuple(drift0[b]))
        _assert_frames(params[b, : want.shape[0]], want, "events entry row %d" % b)
    want, _ = oracle.tracks_generate(oracle.track_config(cfgv), tabs[-1], tuple(drift0[-1]))
    ref = oracle.synthesize(oracle.male_config(44100.0, 1, float_model=1), want)
    assert np.isfinite(ref).all() and n2[-1].item() == ref.size
    assert np.array_equal(a2[-1, : ref.size].cpu().numpy(), ref)


def _launch_voices(plan, tabs, ids, max_frames, drift_in):
    """_launch through gvtm_generate_tracks_voices_device: utterance b under the track configuration of voice ids[b] of
    `plan`; the counts start out 99, as chunk_cases.generate_tracks_chunks' do."""
    import torch
    d_events, d_offsets = events_on_device(tabs)
    b = len(tabs)
    buf = torch.full(((b * max_frames + GUARD_FRAMES) * 16,), SENTINEL, dtype=torch.int32, device=d_events.device).view(torch.float32)
    counts = torch.full((b,), 99, dtype=torch.int32, device=d_events.device)
    d_ids, drift = to_device(np.asarray(ids, dtype=np.int32), np.ascontiguousarray(drift_in, dtype=np.float64).copy())
    plan.generate_tracks_voices_device(d_events, d_offsets, d_ids, b, max_frames, buf, counts, drift, current_stream())
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    return out[: b * max_frames * 16].reshape(b, max_frames, 16), out[b * max_frames * 16:], counts.cpu().numpy(), drift.cpu().numpy()


def test_voices_and_chunks_entries_at_the_walk_edges(tables):
    """The walk's edges through its other two compiles: gvtm_generate_tracks_voices_device and, each list as its
    utterance's one chunk (utt_chunks = 0..9), gvtm_generate_tracks_chunks_device.  Two voices whose track configurations
    have every flag the other way round, alternating inside the wavefronts; lists on both sides of the table next to each
    other and next to a list of one event, a 1,000-event list next to a row whose voice id is outside the table, an empty
    list, and a batch of 9, whose last workgroup holds one row; generators that ran before; cut at 33 frames (one flush of
    the ring and one frame) and at 600.  Every row against the oracle under its voice's configuration, the short rows and
    the row of the bad id untouched, and the two entries bit for bit each other's."""
    cfgvs = [cases.calls("flags16")[6], cases.calls("flags16")[9]]
    assert [c[1:5].tolist() for c in cfgvs] == [[0, 1, 1, 0], [1, 0, 0, 1]]
    plan = g.VoicesPlan(configs(precision=capi.PRECISION_F32, names=VOICES[:2]), 250.0, 0)
    plan.set_voice_tracks([product_config(c) for c in cfgvs])
    names = ["b239", "b240", "b241", "e1", "far1000", "flags16", "e0", "b242", "unset_first"]
    ids = [0, 1, 1, 0, 0, 2, 1, 0, 1]
    bad, short = 5, (3, 6)
    tabs = [tables[n] for n in names]
    assert len(tabs) == 9 and [tabs[b].shape[0] for b in short] == [1, 0]
    drift0 = _states(len(tabs), 18)
    caches = [{}, {}]  # per voice: the oracle walks each list once for both buffer lengths and both entries
    for max_frames in (33, 600):
        got_v = _launch_voices(plan, tabs, ids, max_frames, drift0)
        got_c = generate_tracks_chunks(plan, [[t] for t in tabs], ids, max_frames, drift0)
        for entry, got in (("voices", got_v), ("chunks", got_c)):
            params, guard, counts, drift = got
            what = "%s entry, max_frames %d" % (entry, max_frames)
            for b, v in enumerate(ids):
                if b == bad:
                    continue
                _check_rows(cfgvs[v], tabs[b: b + 1], max_frames, drift0[b: b + 1],
                            (params[b: b + 1], guard, counts[b: b + 1], drift[b: b + 1]), "%s, row %d" % (what, b), caches[v])
            for b in (bad,) + short:
                assert counts[b] == 0, (what, b)
                assert (params[b].view(np.uint32) == SENTINEL).all(), (what, b)
                assert np.array_equal(drift[b].view(np.int64), drift0[b].view(np.int64)), (what, b)
            assert counts[4] > 600 and (counts[[0, 1, 2, 7, 8]] > 33).all()  # both buffers cut rows short
        for x, y in zip(got_v, got_c):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), "max_frames %d: the two entries differ" % max_frames
