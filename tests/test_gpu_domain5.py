"""The model 5 kernels on parameter frames OUTSIDE the editor's ranges (tests/domain5_cases.py), against the oracle, which
tests/test_domain5_cpu.py holds to the real reference bit for bit on the same frames -- in all four code objects of
csrc/vtm_kernel_m5.inc: the double class, the float class and the several-voices variant of each.

One launch per cell.  A launch takes every male case of the table as one batch plus the 3-frame prefixes of three of them
(an S1 and an S30 frication position on the frication-only base, pitch 70): the rows are ragged, and a prefix ends in the
middle of the ramp towards the out-of-range frame.  8 x 242 steps per utterance, a few dozen utterances.

    cells       the double class forced to rows 1 and rows 2; the float class forced to rows 1 (chunk 60) and rows 2
                (chunk 56); the product library with nothing forced, in both classes.
    per utterance   the exact count; the samples -- double class: parity_rules.check_batch (2e-6 of peak, 90 % of the
                samples exact); float class with the case's arguments inside the pinned ranges
                (domain5_cases.float_pinned5): bit for bit, with the oracle's maxabs; float outside the pinned ranges:
                parity_rules.TOL[MIXED], a guard against a wrong branch, not a wrong bit (a share of the frication in the
                wrong section misses by 0.25 % to 99 % of peak); float on a track that enters S1, whose share the kernel
                folds into the tube input one rounding away from the reference (domain5_cases.S1_FLOAT_BAR, with the
                reason): the same bar --; the row zero beyond its count; everything finite.
    voices      male, female, baby and the four 5_male variants (tn_delta, sine, const_mouth, no_modulation) in one plan,
                each configuration's cases shuffled into one launch: every utterance bit for bit its single-voice plan's,
                and its configuration's oracle to the class's rule.
    stream      the male batch through a lockstep stream in pieces of 3, 1 and 4 frames: the one-shot output bit for bit.
    product rule    positions whose section lies outside S1..S30, where the reference is undefined: nothing is injected.
                The constant-position tracks against the oracle on the same frames with fricVol 0 (numerically: a +0 may
                stand for a -0), the two ramps against the guarded oracle, in every cell.
"""
import functools

import numpy as np
import pytest

import domain5_cases as cases
import gama_tts_amd as g
from gama_tts_amd import capi
from parity_rules import TOL, check_batch, peak_err, within
from voice_cases import model5_plan, padded, push_in_pieces

pytestmark = pytest.mark.gpu

PREFIXES = ("fpos_m1.7_F", "fpos_7.8_F", "pitch_70")
# (float class, forced rows; 0: the product library with nothing forced)
CELLS = [(False, 1), (False, 2), (True, 1), (True, 2), (False, 0), (True, 0)]
CELL_IDS = ["%s-%s" % ("float" if f else "double", "rows%d" % r if r else "product") for f, r in CELLS]
VOICE_CONFIGS = list(cases.CONFIGS)  # voice id v of the several-voices plan


def male_batch():
    """[(case, its frames)]: every male case, then the prefixes."""
    full = [(c, cases.track_for(c)) for c in cases.cases_of("male")]
    return full + [(cases.BY_NAME[n], cases.track_for(cases.BY_NAME[n])[:3]) for n in PREFIXES]


@functools.lru_cache(maxsize=None)
def male_reference(float_model):
    return tuple(cases.synthesize_many([("male", float_model, t) for _, t in male_batch()]))


@functools.lru_cache(maxsize=None)
def product_reference(float_model):
    """The oracle's samples of the product-rule cases: const tracks on the frames with fricVol 0, ramps as they are."""
    return tuple(cases.synthesize_many([("male", float_model, cases.track_for(c, neutral=c["form"] == "const"))
                                        for c in cases.PRODUCT_CASES]))


def plan_of(float_class, rows, config="male"):
    voice, overrides = cases.CONFIGS[config]
    return model5_plan(voice, overrides, cases.RATE, cases.CRATE, rows=rows, float_class=float_class)


def check(audio, counts, maxabs, refs, batch, fs, float_class, label, numeric=False):
    """Every utterance of a launch against its reference by the rules of the module docstring; all misses reported.
    batch: [(case, frames)]; numeric: the float class compares values, not bits (+0 == -0)."""
    bad = []
    assert np.isfinite(audio).all() and np.isfinite(maxabs).all(), label
    for b, (ref, (case, track)) in enumerate(zip(refs, batch)):
        name = case["name"] + ("[:%d]" % track.shape[0] if track.shape[0] != cases.FRAMES else "")
        got = audio[b, : ref.size]
        err = peak_err(got, ref)
        exact = float_class and case["float_bar"] is None and cases.float_pinned5(track, fs)
        print("%s %-16s count %5d (%5d) peak-relative error %.3g differing samples %d of %d %s"
              % (label, name, counts[b], ref.size, err, int((got != ref).sum()), ref.size, "exact" if exact else ""))
        if counts[b] != ref.size:
            bad.append((name, "count", int(counts[b]), ref.size))
            continue
        if not float_class:
            try:
                check_batch(audio[b: b + 1], counts[b: b + 1], maxabs[b: b + 1], [ref], False)
            except AssertionError as e:
                bad.append((name, "model 5's bar", err, str(e)[:60]))
        elif exact:
            same = np.array_equal(got, ref) if numeric else np.array_equal(got.view(np.uint32), ref.view(np.uint32))
            if not same or maxabs[b] != (np.abs(ref).max() if ref.size else 0.0):
                bad.append((name, "bits", err))
        else:
            tol = case["float_bar"] or TOL[capi.PRECISION_MIXED]
            if not within(got, ref, tol) or maxabs[b] != np.abs(got).max():
                bad.append((name, "tolerance %g" % tol, err))
        if audio[b, ref.size:].any():
            bad.append((name, "row not zero beyond its count"))
    assert not bad, (label, bad)


@pytest.mark.parametrize("float_class,rows", CELLS, ids=CELL_IDS)
def test_out_of_range_frames_against_the_oracle(float_class, rows):
    plan = plan_of(float_class, rows)
    assert plan.diagnostics == bool(rows)
    batch = male_batch()
    params, frames = padded([t for _, t in batch])
    assert frames.tolist() == [cases.FRAMES] * len(cases.cases_of("male")) + [3] * len(PREFIXES)
    audio, counts, maxabs = plan.synthesize_host(params, frames)
    check(audio, counts, maxabs, male_reference(int(float_class)), batch, plan.info.internal_rate_hz, float_class,
          CELL_IDS[CELLS.index((float_class, rows))])
    plan.close()


@pytest.mark.parametrize("float_class,rows", CELLS, ids=CELL_IDS)
def test_positions_outside_the_tube_inject_nothing(float_class, rows):
    plan = plan_of(float_class, rows)
    batch = [(c, cases.track_for(c)) for c in cases.PRODUCT_CASES]
    params, frames = padded([t for _, t in batch])
    audio, counts, maxabs = plan.synthesize_host(params, frames)
    check(audio, counts, maxabs, product_reference(int(float_class)), batch, plan.info.internal_rate_hz, float_class,
          "outside-" + CELL_IDS[CELLS.index((float_class, rows))], numeric=True)
    plan.close()


@pytest.mark.parametrize("float_class", [False, True], ids=["double", "float"])
def test_a_lockstep_stream_in_uneven_pieces_is_the_one_shot_output(float_class):
    plan = plan_of(float_class, 0)
    male = cases.cases_of("male")
    full = np.stack([cases.track_for(c) for c in male])
    audio, counts, maxabs = plan.synthesize_host(full)
    total = np.full(full.shape[0], cases.FRAMES, dtype=np.int32)
    outs, peaks = push_in_pieces(plan, full, total, (3, 1, 4))
    refs = male_reference(int(float_class))
    for b, case in enumerate(male):
        assert outs[b].size == counts[b] == refs[b].size, case["name"]
        assert np.array_equal(outs[b].view(np.uint32), audio[b, : counts[b]].view(np.uint32)), case["name"]
        assert peaks[b] == maxabs[b], case["name"]
    plan.close()


@pytest.mark.parametrize("float_class", [False, True], ids=["double", "float"])
def test_seven_configurations_in_one_launch(float_class):
    precision = capi.PRECISION_F32 if float_class else capi.PRECISION_F64
    cfgs = []
    for config in VOICE_CONFIGS:
        d = g.read_config_file(cases.model5_cases.voice_files.voice_path(cases.CONFIGS[config][0], True))
        d.update({k: str(v) for k, v in cases.CONFIGS[config][1].items()})
        cfgs.append(g.config5_from_dict(d, cases.RATE, precision))
    plan = g.VoicesPlan(cfgs, cases.CRATE, 0, float_model5=float_class)
    batch = [(v, c) for v, config in enumerate(VOICE_CONFIGS) for c in cases.cases_of(config)]
    order = np.random.default_rng(5).permutation(len(batch))
    batch = [batch[i] for i in order]
    ids = np.array([v for v, _ in batch], dtype=np.int32)
    assert sorted(set(ids.tolist())) == list(range(len(VOICE_CONFIGS))) and (np.diff(ids) != 0).sum() > len(VOICE_CONFIGS)
    utts = [cases.track_for(c) for _, c in batch]
    params, frames = padded(utts)
    audio, counts, maxabs = plan.synthesize_host(params, ids, frames)
    assert np.isfinite(audio).all()
    refs = cases.synthesize_many([(VOICE_CONFIGS[v], int(float_class), t) for (v, _), t in zip(batch, utts)])
    for v, config in enumerate(VOICE_CONFIGS):
        sel = np.flatnonzero(ids == v)
        single = plan_of(float_class, 0, config)
        fs = single.info.internal_rate_hz
        assert fs == plan.voice_info(v).internal_rate_hz, config
        s_audio, s_counts, s_maxabs = single.synthesize_host(params[sel], frames[sel])
        for j, b in enumerate(sel):
            name = (config, batch[b][1]["name"])
            assert counts[b] == s_counts[j] and maxabs[b] == s_maxabs[j], name
            assert np.array_equal(audio[b, : counts[b]].view(np.uint32), s_audio[j, : s_counts[j]].view(np.uint32)), name
        single.close()
        check(audio[sel], counts[sel], maxabs[sel], [refs[b] for b in sel], [(batch[b][1], utts[b]) for b in sel], fs,
              float_class, "voices-%s-%s" % ("float" if float_class else "double", config))
    plan.close()
