"""The kernels on parameter frames OUTSIDE the editor's ranges (tests/domain_cases.py), against the oracle, which
tests/test_domain_cpu.py holds to the real reference bit for bit on the same frames.

One launch per cell.  A launch takes every case of the table as one batch plus the 3-frame prefixes of three of them:
the rows are ragged, and a prefix ends in the middle of the ramp towards the out-of-range frame.

    cells       precision float / fp64 / mixed  x  {SectionDelay 1, SectionDelay 2, the 48-lane layout (30 + 18 tube)}
                x forced rows 1 / 2 / 4, and 8 in float on the 10 + 6 tube (the other rows-8 requests fall back to the
                four-row shape, tests/kernel_shape_cases.py: left out).
                  frication record (csrc/vtm_kernel_v2.inc, fr_compact<CT>()): the COMPACT form (two shares, a zero and the
                    first section's index) in every fp64 and mixed cell, the DENSE form (eight taps and a zero) in every
                    float cell;
                  library fallbacks of the float conversions (far_calls_inline<D, U>()): IN LINE in the rows-4 cells at
                    SectionDelay 1, on both tubes, as cold calls everywhere else.  Only the float cells have such fallbacks.
    per utterance   the exact count; the samples -- float and the case's arguments inside the pinned ranges
                (domain_cases.float_pinned at the cell's internal rate): bit for bit, with the oracle's maxabs; fp64 and
                mixed: parity_rules.within at parity_rules.TOL; float outside the pinned ranges: the mixed bar, a guard
                against a wrong branch, not a wrong bit (one case, fcf_9e5, was measured beyond it on the 30 + 18 tube
                and has a bar of its own, four times the measured error: domain_cases.FCF_9E5_FLOAT_BAR) --; the row zero
                beyond its count; everything finite.
    stream      the batch through a lockstep stream in pieces of 3, 1 and 4 frames: the one-shot output bit for bit.
    voices      male + female in one four-row launch: their single-voice plans bit for bit, and the female utterances the
                female oracle (at ITS internal rate the bandwidth cases are inside tanf's range, 60 kHz stays outside cosf's).
    product     the product library with nothing forced.

Reference model 5 has a table and a module of its own: tests/domain5_cases.py, tests/test_gpu_domain5.py."""
import functools

import numpy as np
import pytest

import domain_cases
import gama_tts_amd as g
import oracle
from gama_tts_amd import capi
from parity_rules import TOL, peak_err, within
from voice_cases import configs, male_plan, oracle_config, padded, push_in_pieces

pytestmark = pytest.mark.gpu

RATE = domain_cases.RATE
TUBES = {"d1": (1, 0), "d2": (2, 0), "lanes48": (1, 1)}  # SectionDelay, tube layout
PRECISIONS = {"f32": capi.PRECISION_F32, "f64": capi.PRECISION_F64, "mixed": capi.PRECISION_MIXED}
PREFIXES = ("fpos_m1.5", "fbw_0.49fs", "pitch_70")
CELLS = [(p, t, rows) for p in PRECISIONS for t in TUBES for rows in (1, 2, 4, 8)
         if rows < 8 or (p == "f32" and t != "lanes48")]


def utterances(fs):
    full = [domain_cases.track_for(c, fs) for c in domain_cases.CASES]
    return full + [domain_cases.track_for(domain_cases.BY_NAME[n], fs)[:3] for n in PREFIXES]


def names():
    return [c["name"] for c in domain_cases.CASES] + [n + "[:3]" for n in PREFIXES]


@functools.lru_cache(maxsize=None)
def reference(delay, layout, float_model):
    """(internal rate, the oracle's samples of every utterance): computed once per configuration and class."""
    fs = float(oracle.derive(oracle.male_config(RATE, delay, layout, float_model=float_model)).sample_rate)
    out = tuple(oracle.synthesize_many([(u, RATE, delay, layout, float_model) for u in utterances(fs)]))
    for r in out:
        r.setflags(write=False)
    return fs, out


def check(audio, counts, maxabs, refs, tracks_, fs, precision, label):
    """Every utterance of a launch against its reference by the rules of the module docstring; all misses reported."""
    bad = []
    assert np.isfinite(audio).all() and np.isfinite(maxabs).all(), label
    for b, (ref, name) in enumerate(zip(refs, names())):
        exact = precision == capi.PRECISION_F32 and domain_cases.float_pinned(tracks_[b], fs)
        tol = TOL[precision]
        if precision == capi.PRECISION_F32 and not exact:
            tol = domain_cases.BY_NAME[name.split("[")[0]]["float_bar"] or TOL[capi.PRECISION_MIXED]
        got = audio[b, : ref.size]
        err = peak_err(got, ref)
        print("%s %-14s count %5d (%5d) peak-relative error %.3g differing samples %d %s"
              % (label, name, counts[b], ref.size, err, int((got != ref).sum()), "exact" if exact else "tol %g" % tol))
        if counts[b] != ref.size:
            bad.append((name, "count", int(counts[b]), ref.size))
            continue
        peak = np.abs(ref).max()
        if exact:
            if not np.array_equal(got.view(np.uint32), ref.view(np.uint32)) or maxabs[b] != peak:
                bad.append((name, "bits", err))
        elif not within(got, ref, tol) or maxabs[b] != np.abs(got).max():
            bad.append((name, "tolerance %g" % tol, err))
        if audio[b, ref.size:].any():
            bad.append((name, "row not zero beyond its count"))
    assert not bad, (label, bad)


@pytest.mark.parametrize("precision,tube,rows", CELLS, ids=["%s-%s-rows%d" % c for c in CELLS])
def test_out_of_range_frames_against_the_oracle(precision, tube, rows):
    delay, layout = TUBES[tube]
    prec = PRECISIONS[precision]
    plan = male_plan(rate=RATE, delay=delay, precision=prec, layout=layout, rows=rows)
    fs, refs = reference(delay, layout, int(prec == capi.PRECISION_F32))
    assert plan.info.internal_sample_rate == fs
    utts = utterances(fs)
    params, frames = padded(utts)
    assert frames.tolist() == [domain_cases.FRAMES] * len(domain_cases.CASES) + [3] * len(PREFIXES)
    audio, counts, maxabs = plan.synthesize_host(params, frames)
    check(audio, counts, maxabs, refs, utts, fs, prec, "%s-%s-rows%d" % (precision, tube, rows))
    plan.close()


def test_a_lockstep_stream_in_uneven_pieces_is_the_one_shot_output():
    plan = male_plan(rate=RATE, precision=capi.PRECISION_F32, diagnostics=True)
    fs, refs = reference(1, 0, 1)
    full = np.stack(utterances(fs)[: len(domain_cases.CASES)])
    audio, counts, maxabs = plan.synthesize_host(full)
    total = np.full(full.shape[0], domain_cases.FRAMES, dtype=np.int32)
    outs, peaks = push_in_pieces(plan, full, total, (3, 1, 4))
    for b, case in enumerate(domain_cases.CASES):
        assert outs[b].size == counts[b] == refs[b].size, case["name"]
        assert np.array_equal(outs[b].view(np.uint32), audio[b, : counts[b]].view(np.uint32)), case["name"]
        assert peaks[b] == maxabs[b], case["name"]
        if case["float_pinned"]:
            assert np.array_equal(outs[b].view(np.uint32), refs[b].view(np.uint32)), case["name"]
    plan.close()


def test_two_voices_in_one_four_row_launch():
    voices = ("male", "female")
    cfgs = configs(RATE, 1, capi.PRECISION_F32, 0, names=voices)
    plan = g.VoicesPlan(cfgs, 250.0, 0, diagnostics=True, rows=4)
    fs = float(plan.voice_info(0).internal_sample_rate)
    utts = utterances(fs)
    params, frames = padded(utts)
    ids = (np.arange(len(utts)) % 3 == 1).astype(np.int32)  # male, female, male | male, female, male | ...
    ids[-len(PREFIXES):] = [1, 0, 1]
    audio, counts, maxabs = plan.synthesize_host(params, ids, frames)
    assert np.isfinite(audio).all()
    for v, voice in enumerate(voices):
        sel = np.flatnonzero(ids == v)
        single = g.Plan(cfgs[v], 250.0, 0, diagnostics=True, rows=4)
        s_audio, s_counts, s_maxabs = single.synthesize_host(params[sel], frames[sel])
        for j, b in enumerate(sel):
            assert counts[b] == s_counts[j] and maxabs[b] == s_maxabs[j], (voice, names()[b])
            assert np.array_equal(audio[b, : counts[b]].view(np.uint32), s_audio[j, : s_counts[j]].view(np.uint32)), (voice, names()[b])
            assert not audio[b, counts[b]:].any(), (voice, names()[b])
        single.close()
    fem_fs = float(plan.voice_info(1).internal_sample_rate)
    fem = oracle_config("female", RATE, 1, 0, capi.PRECISION_F32)
    assert float(oracle.derive(fem).sample_rate) == fem_fs
    bad = []
    for b in np.flatnonzero(ids == 1):
        ref = oracle.synthesize(fem, utts[b])
        assert np.isfinite(ref).all() and counts[b] == ref.size, names()[b]
        got = audio[b, : ref.size]
        if domain_cases.float_pinned(utts[b], fem_fs):
            ok = np.array_equal(got.view(np.uint32), ref.view(np.uint32)) and maxabs[b] == np.abs(ref).max()
        else:
            ok = within(got, ref, TOL[capi.PRECISION_MIXED])
        print("female %-14s peak-relative error %.3g" % (names()[b], peak_err(got, ref)))
        if not ok:
            bad.append((names()[b], peak_err(got, ref)))
    assert not bad, bad
    plan.close()


def test_the_product_library_with_nothing_forced():
    plan = g.Plan(g.config_from_dict(g.read_config_file(oracle.VOICE_MALE), RATE, 1, capi.PRECISION_F32), 250.0, 0)
    assert not plan.diagnostics
    fs, refs = reference(1, 0, 1)
    utts = utterances(fs)
    params, frames = padded(utts)
    audio, counts, maxabs = plan.synthesize_host(params, frames)
    check(audio, counts, maxabs, refs, utts, fs, capi.PRECISION_F32, "product-f32-d1")
    plan.close()
