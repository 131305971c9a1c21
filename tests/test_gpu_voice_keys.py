"""The kernels on the voice-configuration keys that every other test leaves at the male voice's value
(tests/voice_key_cases.py; tests/test_voice_keys_cpu.py holds the oracle at these sets to the real reference and the host
designs to the oracle's).

One voice: every set through the one-row and the four-row shape of every cell (precision x tube x converter direction)
and, for `acoustics`, through the product library with nothing forced, against the oracle under parity_rules.TOL.
Several voices: the male voice and the seven sets in one plan, in two orders, so that a kernel that read a constant from
another voice's block, or from the by-value floats of voice 0, gives some utterance another voice's samples: every
utterance bit for bit a single-voice plan's at the same rows, and within the precision's rule of the oracle; the same
batch through streams, bit for bit the one-shot launch.  Reference model 5: its two sets in both classes, alone and in
plans of three voices.

All on one 24-frame track and its cuts at 0, 1, 2 and 13 frames; 79 and 87 steps per frame next to the male voice's 80."""
import functools

import numpy as np
import pytest

import gama_tts_amd as g
from gama_tts_amd import capi
import model5_cases
import oracle
import shape_matrix_cases
import voice_key_cases as cases
import voices_matrix_cases
from parity_rules import TOL, check_batch, within
from voice_cases import male_plan, model5_plan, push_in_pieces

pytestmark = pytest.mark.gpu

CELLS = pytest.mark.parametrize("cell", cases.CELLS, ids=cases.CELL_IDS)
ORDERS = pytest.mark.parametrize("order", list(cases.ORDERS))


def config_of(cell, name):
    d = g.read_config_file(oracle.VOICE_MALE)
    d.update({k: str(v) for k, v in cases.overrides_of(name).items()})
    return g.config_from_dict(d, cell.rate, cell.delay, cell.precision, cell.layout)


def config5_of(name, float_class):
    d = g.read_config_file(oracle.VOICE5_MALE)
    d.update({k: str(v) for k, v in cases.overrides_of(name).items()})
    return g.config5_from_dict(d, cases.RATE5, capi.PRECISION_F32 if float_class else capi.PRECISION_F64)


@functools.lru_cache(maxsize=None)
def oracle_ref(name, rate, delay, layout, float_model, frames):
    """The oracle's samples of the track cut to `frames` under a voice of the table; computed once, read-only."""
    out = oracle.synthesize(oracle.male_config(rate, delay, layout, float_model, **cases.overrides_of(name)), cases.track()[:frames])
    out.setflags(write=False)
    return out


def ref_of(cell, name, frames):
    return oracle_ref(name, cell.rate, cell.delay, cell.layout, cell.float_model, int(frames))


@functools.lru_cache(maxsize=None)
def oracle5_ref(name, float_model, frames):
    cfg = model5_cases.voice_oracle_config("male", cases.RATE5, float_model, cases.overrides_of(name))
    out, _ = oracle.synthesize5(cfg, cases.track()[:frames])
    out.setflags(write=False)
    return out


def check_against_oracle(cell, name, audio, counts, maxabs, frames):
    for b, f in enumerate(frames):
        ref = ref_of(cell, name, f)
        assert counts[b] == ref.size, (name, b)
        got = audio[b, : ref.size]
        assert within(got, ref, TOL[cell.precision]), (name, b, int(f))
        assert maxabs[b] == (np.abs(got).max() if ref.size else 0.0), (name, b)


def forced_rows(cell):
    """One row, and four where the cell's four-row shape launches: two where shape_matrix_cases says four fall back."""
    return 1, (2 if cases.shape_matrix_id(cell, 4) in shape_matrix_cases.FALL_BACK else 4)


# ---- one voice ----------------------------------------------------------------------------------------------------------------

@CELLS
def test_one_voice_every_set(cell):
    params, frames = cases.batch()
    for rows in forced_rows(cell):
        for name in cases.SETS:
            plan = male_plan(cases.SETS[name], cell.rate, cell.delay, precision=cell.precision, layout=cell.layout, rows=rows)
            assert plan.diagnostics and shape_matrix_cases.launch_shape(plan, len(frames))[0] == rows, (name, rows)
            audio, counts, maxabs = plan.synthesize_host(params, frames)
            check_against_oracle(cell, name, audio, counts, maxabs, frames)
            assert np.array_equal(audio[5], audio[0])  # the two whole tracks, in different workgroups or rows
            plan.close()


@CELLS
def test_one_voice_in_the_shape_the_product_picks(cell):
    params, frames = cases.batch()
    plan = male_plan(cases.SETS["acoustics"], cell.rate, cell.delay, precision=cell.precision, layout=cell.layout)
    assert not plan.diagnostics
    assert plan.info.control_steps == cases.STEPS["acoustics"][cases.steps_index(cell)]
    audio, counts, maxabs = plan.synthesize_host(params, frames)
    check_against_oracle(cell, "acoustics", audio, counts, maxabs, frames)


# ---- several voices -----------------------------------------------------------------------------------------------------------

def names_of(order):
    return [cases.VOICE_NAMES[i] for i in cases.ORDERS[order]]


def singles_of(cfgs, params, ids, frames, rows, **kind):
    """Every utterance through a single-voice plan of its voice, the diagnostics library's forced to `rows`: the same batch
    (the other voices' utterances as filler), that voice's rows kept -> {b: (samples, maxabs)}."""
    out = {}
    for v, cfg in enumerate(cfgs):
        plan = g.Plan(cfg, cases.CRATE, 0, diagnostics=True, rows=rows, **kind)
        audio, counts, maxabs = plan.synthesize_host(params, frames)
        for b in np.nonzero(ids == v)[0]:
            out[int(b)] = (audio[b, : counts[b]].copy(), float(maxabs[b]))
        plan.close()
    return out


def assert_as_singles(audio, counts, maxabs, singles, what):
    for b, (ref, peak) in singles.items():
        assert counts[b] == ref.size, (what, b)
        assert np.array_equal(audio[b, : ref.size], ref), (what, b)
        assert maxabs[b] == peak, (what, b)


@ORDERS
@CELLS
def test_eight_voices_in_one_launch(cell, order):
    names = names_of(order)
    cfgs = [config_of(cell, n) for n in names]
    params, ids, frames = cases.voices_batch(len(names))
    for forced in (0, 2, 4):
        # forced 0: the product library at its own choice of rows, which a diagnostics plan with nothing forced answers
        diag = g.VoicesPlan(cfgs, cases.CRATE, 0, diagnostics=True, rows=forced)
        rows = voices_matrix_cases.voices_launch_shape(diag, len(ids))[0]
        assert forced == 0 or rows == forced or (forced == 4 and rows == 2), (forced, rows)
        plan = diag if forced else g.VoicesPlan(cfgs, cases.CRATE, 0)
        assert bool(forced) == plan.diagnostics
        assert len({plan.voice_info(v).control_steps for v in range(len(names))}) == 3  # internal rates that differ
        audio, counts, maxabs = plan.synthesize_host(params, ids, frames)
        assert_as_singles(audio, counts, maxabs, singles_of(cfgs, params, ids, frames, rows), (forced, rows))
        for b in range(len(ids)):
            ref = ref_of(cell, names[ids[b]], frames[b])
            assert counts[b] == ref.size == plan.voice_output_count(int(ids[b]), int(frames[b])), (forced, b)
            assert within(audio[b, : ref.size], ref, TOL[cell.precision]), (forced, b, names[ids[b]])
            assert not audio[b, ref.size:].any(), (forced, b)
        plan.close()
        diag.close()


@ORDERS
@pytest.mark.parametrize("cell", cases.STREAM_CELLS, ids=[c.name for c in cases.STREAM_CELLS])
def test_eight_voices_through_streams(cell, order):
    names = names_of(order)
    plan = g.VoicesPlan([config_of(cell, n) for n in names], cases.CRATE, 0)
    params, ids, ragged = cases.voices_batch(len(names))
    whole = np.broadcast_to(cases.track(), (len(ids), cases.FRAMES, 16)).copy()
    for batch, total in ((whole, np.full(len(ids), cases.FRAMES, dtype=np.int32)), (params, ragged)):
        audio, counts, _ = plan.synthesize_host(batch, ids, total)
        samples, maxabs = push_in_pieces(plan, batch, total, cases.STREAM_PIECES, voice_ids=ids)
        for b in range(len(ids)):
            assert samples[b].size == counts[b], b
            assert np.array_equal(samples[b], audio[b, : counts[b]]), (b, names[ids[b]], int(total[b]))
            assert maxabs[b] == (np.abs(samples[b]).max() if samples[b].size else 0.0), b


# ---- reference model 5 ----------------------------------------------------------------------------------------------------------

CLASSES = pytest.mark.parametrize("float_class", [False, True], ids=["double", "float"])


def exact_share(audio, refs):
    return min(float((audio[b, : r.size] == r).mean()) for b, r in enumerate(refs) if r.size >= 200)


@CLASSES
@pytest.mark.parametrize("name", list(cases.SETS5))
def test_model5_sets(name, float_class):
    params, frames = cases.batch()
    plan = model5_plan("male", cases.SETS5[name], cases.RATE5, cases.CRATE, float_class=float_class)
    audio, counts, maxabs = plan.synthesize_host(params, frames)
    refs = [oracle5_ref(name, int(float_class), int(f)) for f in frames]
    print("%s %s: smallest share of bit-identical samples %.4f" % (name, "float" if float_class else "double", exact_share(audio, refs)))
    check_batch(audio, counts, maxabs, refs, float_class)


@CLASSES
def test_model5_three_voices_in_one_launch(float_class):
    cfgs = [config5_of(n, float_class) for n in cases.VOICE_NAMES5]
    plan = g.VoicesPlan(cfgs, cases.CRATE, 0, float_model5=float_class)
    params, ids, frames = cases.voices_batch(len(cfgs))
    audio, counts, maxabs = plan.synthesize_host(params, ids, frames)
    assert plan.voice_info(1).control_steps != plan.voice_info(0).control_steps == plan.voice_info(2).control_steps
    for v, cfg in enumerate(cfgs):
        sel = np.nonzero(ids == v)[0]
        single = g.Plan(cfg, cases.CRATE, 0, float_model5=float_class)
        s_audio, s_counts, s_maxabs = single.synthesize_host(params[sel], frames[sel])
        for j, b in enumerate(sel):
            assert counts[b] == s_counts[j] and maxabs[b] == s_maxabs[j], (v, b)
            assert np.array_equal(audio[b, : counts[b]], s_audio[j, : s_counts[j]]), (v, b)
        check_batch(audio[sel], counts[sel], maxabs[sel], [oracle5_ref(cases.VOICE_NAMES5[v], int(float_class), int(f)) for f in frames[sel]],
                    float_class)
