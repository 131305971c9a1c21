"""The float class of reference model 5 on the GPU (gvtm_plan_create_model5_float, csrc/vtm_kernels_m5f.hip) on all five
5_male variants, and both classes of model 5 at the limits of the sample-rate converter.

tests/test_gpu_model5_float.py holds the float kernel to bit identity on the male voice alone: 242 internal steps per
250 Hz frame (even, so every chunk tail is even) at 60.4 kHz.  The other voices (tests/golden/voice5_*.txt) change every
derived float constant, the chunk tails, the output samples per chunk and sink block, and the frames a stream holds back:

    voice        internal rate   steps / frame   last chunk of one frame, chunk 60 / 56   stream granule (frames)
    male          60 411.43 Hz   242             2 / 18                                   2
    female        70 480 Hz      282             42 / 2                                   2
    large_child   84 576 Hz      338             38 / 2                                   2
    small_child  105 720 Hz      423 (odd)       3 / 31                                   4
    baby         140 960 Hz      564             24 / 4                                   1

The bar is test_gpu_model5_float.py's: parity_rules.within(got, ref, TOL[PRECISION_F32]) -- bit identity -- with sample
counts exact and maxabs == abs(out).max().  References are the vectors of the real class (tests/golden/voices5f_golden.npz)
and the float oracle, which tests/test_oracle5f_voices_vs_golden.py holds to those vectors.  Every float test runs in the
shape the product picks (chunk 60 up to 256 utterances) and with chunk 56 forced (a diagnostics plan, rows 2).

The converter limits -- a down-sampling pad of 96, the largest a plan accepts and what the kernel's ring is sized for, and
an output rate of 3 x the internal rate -- are run in both classes: the float class bit for bit, the double class
(gvtm_plan_create_model5; rows 2 is its two-utterance workgroup) to parity_rules.check_model5, test_gpu_model5.py's bar."""
import functools
import hashlib

import numpy as np
import pytest

from gama_tts_amd import capi
import model5_cases as cases
import oracle
import tracks
from parity_rules import TOL, TOL5, check_batch, check_model5, within
from voice_cases import model5_plan, padded, push_in_pieces
from voice_files import VOICES

pytestmark = pytest.mark.gpu

BIT_IDENTICAL = TOL[capi.PRECISION_F32]
SHAPES = pytest.mark.parametrize("rows", [0, 2], ids=["product_shape", "chunk56"])
# (voice, output rate, control rate, steps per frame): chunk 60 exactly, and steps that leave tails of 10 / 31 / 45 steps
CONTROL_RATE_CASES = [("male", 16000.0, 1000.0, 60), ("female", 16000.0, 1000.0, 70), ("small_child", 22050.0, 500.0, 211),
                      ("baby", 32000.0, 200.0, 705)]


# a float model-5 plan of a voice on device 0 (rows 2: a diagnostics plan forced to chunk 56); model5_plan itself gives the
# double class (rows 2: a diagnostics plan forced to two utterances per workgroup)
float_plan = functools.partial(model5_plan, float_class=True)


_refs = {}


def oracle_refs(key, voice, rate, crate, utterances, float_model=1):
    """The oracle's output for a list of utterances, computed once per `key` and shared by the shapes (read-only)."""
    if key not in _refs:
        cfg = cases.voice_oracle_config(voice, rate, float_model)
        refs = [oracle.synthesize5(cfg, u, crate)[0] for u in utterances]
        for r in refs:
            r.setflags(write=False)
        _refs[key] = refs
    return _refs[key]


# ---- reference vectors --------------------------------------------------------------------------------------------------

@SHAPES
@pytest.mark.parametrize("case", cases.FLOAT_CASES, ids=lambda c: c["name"])
def test_reference_vectors(case, rows, golden):
    """Every float vector of voices5f_golden.npz, one utterance per launch: count and SHA-256, then the full, strided or
    tail samples (the tail of an overrun case covers the extra lap of the ring)."""
    data = cases.load("voices5f")
    m = data["manifest"][case["name"]]
    tr = cases.track_for(case, golden)
    plan = float_plan(case["voice"], case["overrides"], case["rate"], case["crate"], rows)
    assert plan.info.model5 == 1 and plan.info.precision == capi.PRECISION_F32
    assert plan.info.control_steps * tr.shape[0] == m["steps"]
    audio, counts, maxabs = plan.synthesize_host(tr[None])
    assert counts[0] == m["n"] == plan.output_count(tr.shape[0])
    out = audio[0, : m["n"]]
    for got, key in cases.stored(case, out):
        assert within(got, data[key], BIT_IDENTICAL), key
    assert hashlib.sha256(out.tobytes()).hexdigest() == m["sha256"]
    assert maxabs[0] == np.abs(out).max() == np.float32(m["maxabs"])


# ---- ragged batches, special frames, control rates against the float oracle ----------------------------------------------

RAGGED_FRAMES = [0, 1, 2, 3, 4, 5, 7, 13, 25, 40]


def ragged_utterances(voice):
    """1 to 5 frames of small_child put 1 to 5 x 423 steps through both chunk lengths (last chunks of 3, 6, 9, 12, 15 steps
    at chunk 60; 31, 6, 37, 12, 43 at chunk 56); its 47 frames are 355 x 56 + 1 steps: a one-step last chunk."""
    params = tracks.random_tracks(len(RAGGED_FRAMES), 40, seed0=7000, consonant_heavy=True)
    us = [params[b, :f] for b, f in enumerate(RAGGED_FRAMES)]
    if voice == "small_child":
        assert (47 * cases.STEPS_PER_FRAME[voice]) % 56 == 1
        us.append(tracks.random_track(47, 7000 + len(RAGGED_FRAMES), True))
    return us


@SHAPES
@pytest.mark.parametrize("voice", VOICES)
def test_ragged_batch_against_the_float_oracle(voice, rows):
    us = ragged_utterances(voice)
    refs = oracle_refs(("ragged", voice), voice, cases.RATE, cases.CRATE, us)
    assert all(np.isfinite(r).all() for r in refs)
    params, frames = padded(us)
    check_batch(*float_plan(voice, rows=rows).synthesize_host(params, frames), refs, True)


@SHAPES
@pytest.mark.parametrize("voice", VOICES)
def test_special_case_frames(voice, rows):
    """tracks.edge_track (volumes 0 / 60 dB, frication at the first / last section, radii at the floor, velum 0, pitch and
    band-pass extremes) alone, and between two random utterances."""
    edge = tracks.edge_track(48)
    us = [tracks.random_track(48, 3, True), edge, tracks.random_track(31, 4, True)]
    refs = oracle_refs(("edge", voice), voice, cases.RATE, cases.CRATE, us)
    assert np.isfinite(refs[1]).all()
    plan = float_plan(voice, rows=rows)
    check_batch(*plan.synthesize_host(edge[None]), [refs[1]], True)
    params, frames = padded(us)
    check_batch(*plan.synthesize_host(params, frames), refs, True)


@SHAPES
@pytest.mark.parametrize("voice,rate,crate,steps", CONTROL_RATE_CASES, ids=lambda v: str(v))
def test_control_rates(voice, rate, crate, steps, rows):
    tr = tracks.random_track(9, 7100, True)
    plan = float_plan(voice, None, rate, crate, rows)
    assert plan.info.control_steps == steps
    refs = oracle_refs(("crate", voice, rate, crate), voice, rate, crate, [tr])
    check_batch(*plan.synthesize_host(tr[None]), refs, True)


def test_product_library_beyond_256_utterances_of_small_child():
    """257 utterances through libgama_vtm.so with nothing forced (the chunk-56 shape): a pool of 8 ragged tracks tiled,
    every pool member against the oracle, every copy equal to its first occurrence."""
    pool_f = np.array([12, 0, 7, 1, 12, 5, 3, 9], dtype=np.int32)
    pool = tracks.random_tracks(len(pool_f), 12, seed0=7200, consonant_heavy=True)
    batch = 257
    idx = np.arange(batch) % len(pool_f)
    audio, counts, maxabs = float_plan("small_child").synthesize_host(pool[idx], pool_f[idx])
    refs = oracle_refs(("pool", "small_child"), "small_child", cases.RATE, cases.CRATE, [pool[t, : pool_f[t]] for t in range(len(pool_f))])
    check_batch(audio, counts, maxabs, refs, True)
    for b in range(len(pool_f), batch):
        assert counts[b] == counts[b % len(pool_f)] and np.array_equal(audio[b], audio[b % len(pool_f)]), b
        assert maxabs[b] == maxabs[b % len(pool_f)]


# ---- streams ------------------------------------------------------------------------------------------------------------

@SHAPES
@pytest.mark.parametrize("voice", ["small_child", "large_child"])
def test_stream_pieces_equal_the_one_shot_samples(voice, rows):
    """A float stream holds frames back until the steps fill whole chunks and sink blocks: 4 frames of small_child (423
    steps), 2 of large_child."""
    total = np.array([33, 20, 8], dtype=np.int32)
    batch = tracks.random_tracks(3, 33, seed0=7300, consonant_heavy=True)
    plan = float_plan(voice, rows=rows)
    one, c1, m1 = plan.synthesize_host(batch, total)
    got, maxabs = push_in_pieces(plan, batch, total, (7, 1, 25))
    refs = oracle_refs(("stream", voice), voice, cases.RATE, cases.CRATE, [batch[b, : total[b]] for b in range(3)])
    for b in range(3):
        assert got[b].size == c1[b] and np.array_equal(got[b], one[b, : c1[b]]), b
        assert maxabs[b] == m1[b]
        assert within(got[b], refs[b], BIT_IDENTICAL), b


@SHAPES
def test_stream_finish_on_a_flush_overrun_of_female(rows):
    """167 frames at 44.1 kHz: finish converts the extra lap of the ring, as the one-shot launch does."""
    f, rate = cases.OVERRUN_FRAMES["female"], cases.OVERRUN_RATE["female"]
    track = tracks.random_track(f, 7400, True)
    plan = float_plan("female", rate=rate, rows=rows)
    whole, counts, peak = plan.synthesize_host(track[None])
    got, maxabs = push_in_pieces(plan, track[None], np.array([f], dtype=np.int32), (7, 1, 25, 134))
    assert got[0].size == counts[0] == plan.output_count(f) > plan.output_count(f + 1)
    assert np.array_equal(got[0], whole[0, : counts[0]]) and maxabs[0] == peak[0]
    assert within(got[0], oracle_refs(("stream_ovr",), "female", rate, cases.CRATE, [track])[0], BIT_IDENTICAL)


# ---- converter limits, float class ----------------------------------------------------------------------------------------

LIMIT_RAGGED_FRAMES = [0, 1, 12, 30]
PAD96 = [(v, r) for v, r, what in cases.LIMITS if what == "pad96"]


def limit_utterances():
    params = tracks.random_tracks(len(LIMIT_RAGGED_FRAMES), 30, seed0=7500, consonant_heavy=True)
    return [params[b, :f] for b, f in enumerate(LIMIT_RAGGED_FRAMES)]


@SHAPES
@pytest.mark.parametrize("voice,rate", PAD96, ids=lambda v: str(v))
def test_pad_96_in_a_ragged_batch(voice, rate, rows):
    us = limit_utterances()
    plan = float_plan(voice, rate=rate, rows=rows)
    assert plan.info.pad_size == cases.MAX_PAD
    params, frames = padded(us)
    check_batch(*plan.synthesize_host(params, frames), oracle_refs(("pad96", voice), voice, rate, cases.CRATE, us), True)


def test_limit_plans_sit_on_the_limits():
    for voice, rate, what in cases.LIMITS:
        info = float_plan(voice, rate=rate).info
        if what == "pad96":
            assert info.pad_size == cases.MAX_PAD and info.upsampling == 0
        else:
            assert info.upsampling == 1 and np.float32(rate) / np.float32(info.internal_rate_hz) == np.float32(3.0)


# ---- converter limits, double class (VocalTractModel5<double,1>: parity_rules.check_model5) ------------------------------

@SHAPES
@pytest.mark.parametrize("case", cases.DOUBLE_CASES, ids=lambda c: c["name"])
def test_double_class_reference_vectors_at_the_converter_limits(case, rows, golden):
    data = cases.load("voices5f")
    m = data["manifest"][case["name"]]
    tr = cases.track_for(case, golden)
    plan = model5_plan(case["voice"], case["overrides"], case["rate"], case["crate"], rows)
    assert plan.info.model5 == 1 and plan.info.precision == capi.PRECISION_F64
    assert abs(plan.info.internal_rate_hz - m["fs"]) < 1e-6
    assert plan.info.control_steps * tr.shape[0] == m["steps"]
    if "pad96" in case["name"]:
        assert plan.info.pad_size == cases.MAX_PAD
    else:
        assert 2.999 < case["rate"] / plan.info.internal_rate_hz <= 3.0
    audio, counts, maxabs = plan.synthesize_host(tr[None])
    assert counts[0] == m["n"] == plan.output_count(tr.shape[0])
    out = audio[0, : m["n"]]
    check_model5(out, data[case["name"] + "__out"], False, m["maxabs"])
    assert maxabs[0] == pytest.approx(m["maxabs"], rel=10 * TOL5, abs=1e-12)
    assert maxabs[0] == np.abs(out).max()


@SHAPES
@pytest.mark.parametrize("voice,rate", PAD96, ids=lambda v: str(v))
def test_double_class_pad_96_in_a_ragged_batch(voice, rate, rows):
    us = limit_utterances()
    plan = model5_plan(voice, rate=rate, rows=rows)
    assert plan.info.pad_size == cases.MAX_PAD
    params, frames = padded(us)
    refs = oracle_refs(("pad96_double", voice), voice, rate, cases.CRATE, us, float_model=0)
    check_batch(*plan.synthesize_host(params, frames), refs, False)
