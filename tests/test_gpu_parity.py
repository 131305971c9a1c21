"""Parity of the HIP path (through the C ABI) with the reference vectors and the oracle.

Tolerance: the metric is max|gpu - ref| / max|ref| per utterance (SURVEY.md hard part 6;
a per-sample relative error is meaningless at zero crossings).
  * fp64 path: 1e-9  (the reference itself only reproduces to 1.6e-8 across compilers, E9).  Both sides
    are float32 samples, so a double-level difference of 1e-13 can still flip the rounding of a sample:
    a sample may therefore also differ by one float32 ulp of itself (6e-8 of the sample; on batch 256 of
    configs[2], 251 utterances are bit-identical and the rest carry a handful of such flips,
    profiles/r01d_config3_parity.json).
  * mixed path: 1e-5 (BASELINE.json north_star)
Sample counts are exact in both.  The rule itself is parity_rules.within, the tolerances parity_rules.TOL.
"""
import numpy as np
import pytest

from gama_tts_amd import capi
import golden_cases
import oracle
import tracks
from parity_rules import TOL, peak_err, within
from voice_cases import male_plan

pytestmark = pytest.mark.gpu

TOL_F64, TOL_MIXED = TOL[capi.PRECISION_F64], TOL[capi.PRECISION_MIXED]


@pytest.mark.parametrize("precision,tol", [(capi.PRECISION_F64, TOL_F64), (capi.PRECISION_MIXED, TOL_MIXED)],
                         ids=["f64", "mixed"])
@pytest.mark.parametrize("case", [c for c in golden_cases.CASES if not c.get("float_model")], ids=lambda c: c["name"])
def test_reference_vectors(case, precision, tol, golden):
    m = golden["manifest"][case["name"]]
    tr = golden_cases.track_for(case, golden)
    plan = male_plan(case["overrides"], case["rate"], case["delay"], case["crate"], precision, case.get("layout", 0))
    assert plan.info.internal_sample_rate == int(m["fs"])
    assert plan.output_count(tr.shape[0]) == m["n"]
    audio, counts, maxabs = plan.synthesize_host(tr[None])
    assert counts[0] == m["n"]
    out = audio[0]
    scale = m["maxabs"] if m["maxabs"] > 0 else 1.0
    if case["store"] == "full":
        ref = golden[case["name"] + "__out"]
        assert within(out, ref, tol, scale), peak_err(out, ref)
    else:
        ref = golden[case["name"] + "__strided"]
        assert within(out[:: golden_cases.DIGEST_STRIDE], ref, tol, scale)
        assert abs(float(out.astype(np.float64).sum()) - m["sum"]) <= 50 * max(tol, 1e-8) * scale * m["n"] ** 0.5 + 1e-12
    assert maxabs[0] == pytest.approx(m["maxabs"], rel=max(10 * tol, 2e-7), abs=1e-12)


@pytest.mark.parametrize("delay", [1, 2, 3])
def test_random_batch_against_oracle(delay):
    params = tracks.random_tracks(12, 40, seed0=300 + delay, consonant_heavy=True)
    plan = male_plan(delay=delay)
    audio, counts, _ = plan.synthesize_host(params)
    ref = oracle.synthesize_batch(oracle.male_config(44100.0, delay), params)
    assert audio.shape == ref.shape and (counts == ref.shape[1]).all()
    for b in range(params.shape[0]):
        assert within(audio[b], ref[b], TOL_F64), peak_err(audio[b], ref[b])


def test_ragged_and_empty_utterances():
    frames = np.array([0, 1, 7, 40, 33, 40, 2, 19], dtype=np.int32)
    params = tracks.random_tracks(len(frames), 40, seed0=77)
    plan = male_plan()
    audio, counts, maxabs = plan.synthesize_host(params, frames)
    cfg = oracle.male_config()
    for b, f in enumerate(frames):
        ref = oracle.synthesize(cfg, params[b, :f]) if f else np.zeros(oracle.output_count(cfg, 0), np.float32)
        assert counts[b] == ref.size == plan.output_count(int(f))
        assert within(audio[b, : ref.size], ref, TOL_F64), peak_err(audio[b, : ref.size], ref)
    assert maxabs[0] == 0.0


def test_normalize_matches_reference_scaling():
    import torch
    params = tracks.random_tracks(3, 30, seed0=5)
    plan = male_plan()
    n = plan.output_count(30)
    dev = torch.device("cuda:0")
    d_params = torch.from_numpy(params).to(dev)
    d_audio = torch.zeros((3, n), dtype=torch.float32, device=dev)
    d_counts = torch.zeros(3, dtype=torch.int64, device=dev)
    d_max = torch.zeros(3, dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    plan.synthesize_device(d_params, 3, 30, d_audio, n, None, d_counts, d_max, stream)
    d_f32 = torch.zeros_like(d_audio)
    d_i16 = torch.zeros((3, n), dtype=torch.int16, device=dev)
    d_scale = torch.zeros(3, dtype=torch.float32, device=dev)
    plan.normalize_device(d_audio, 3, n, d_max, d_counts, d_out_f32=d_f32, d_scales=d_scale, stream=stream)
    plan.normalize_device(d_audio, 3, n, d_max, d_counts, d_out_i16=d_i16, stream=stream)
    torch.cuda.synchronize()
    audio = d_audio.cpu().numpy()
    for b in range(3):
        # integer / elementwise float work on the SAME float32 samples: exact, whatever precision produced them
        # (the restatement below is pinned to WAV files the reference wrote, tests/test_oracle_vs_golden.py)
        scale = np.float32(oracle.output_scale(audio[b]))
        assert np.float32(d_scale[b].item()) == scale
        assert np.array_equal(d_f32[b].cpu().numpy(), audio[b] * scale)
        # WAVEFileWriter.cpp:122-125: round(x * 32767)
        p = (audio[b] * scale) * np.float32(32767.0)
        want = (np.sign(p) * np.floor(np.abs(p) + np.float32(0.5))).astype(np.int16)  # std::round
        assert np.array_equal(d_i16[b].cpu().numpy(), want)


def test_full_size_properties_config2():
    """BASELINE.json configs[1]: batch 256 x 500 frames.  Size-independent checks:
    exact sample counts, run-to-run determinism, independence from batch neighbours,
    causality (a prefix track reproduces the head of the long one), peak bookkeeping,
    plus a spot check of a few utterances against the oracle."""
    params = tracks.random_tracks(256, 500, seed0=1000)
    plan = male_plan()
    audio, counts, maxabs = plan.synthesize_host(params)
    assert audio.shape == (256, 88108) and (counts == 88108).all()
    audio2, _, _ = plan.synthesize_host(params)
    assert np.array_equal(audio, audio2)
    assert np.array_equal(maxabs, np.abs(audio).max(axis=1))
    perm = np.random.default_rng(0).permutation(256)
    audio3, _, _ = plan.synthesize_host(params[perm][:64])
    assert np.array_equal(audio3, audio[perm][:64])
    # causality: the first 200 frames alone give the same samples until the SRC window reaches
    # frame 199 (whose interpolation target differs: frame 200 there, its own copy here)
    head, _, _ = plan.synthesize_host(params[:8, :200])
    safe = int((199 * 80 - 26) * 44100 / 20034) - 2
    assert np.array_equal(head[:, :safe], audio[:8, :safe])
    cfg = oracle.male_config()
    for b in (0, 101, 255):
        assert within(audio[b], oracle.synthesize(cfg, params[b]), TOL_F64), peak_err(audio[b], oracle.synthesize(cfg, params[b]))


@pytest.mark.parametrize("rows,precision,tol", [(2, capi.PRECISION_F64, TOL_F64), (4, capi.PRECISION_F64, TOL_F64),
                                                  (2, capi.PRECISION_MIXED, TOL_MIXED), (4, capi.PRECISION_MIXED, TOL_MIXED)])
@pytest.mark.parametrize("delay", [1, 3])
def test_multi_row_workgroups(rows, precision, tol, delay):
    """Several utterances per workgroup (one DPP row each in the serial wavefronts), ragged
    lengths, a batch that does not fill the last workgroup."""
    frames = np.array([40, 0, 17, 33, 40, 1, 25, 40, 8, 39, 40], dtype=np.int32)
    params = tracks.random_tracks(len(frames), 40, seed0=900 + rows, consonant_heavy=True)
    plan = male_plan(delay=delay, precision=precision, rows=rows)
    audio, counts, maxabs = plan.synthesize_host(params, frames)
    cfg = oracle.male_config(44100.0, delay)
    for b, f in enumerate(frames):
        ref = oracle.synthesize(cfg, params[b, :f]) if f else np.zeros(oracle.output_count(cfg, 0), np.float32)
        assert counts[b] == ref.size
        assert within(audio[b, : ref.size], ref, tol), peak_err(audio[b, : ref.size], ref)
        assert maxabs[b] == np.abs(audio[b, : ref.size]).max()


@pytest.mark.parametrize("frames", [48, 96, 97, 3, 600])
def test_one_step_per_frame_and_chunk_aligned_lengths(frames):
    """The plugin's mode of operation (control rate == internal rate, one frame per step) with
    lengths that are exact multiples of the kernel's chunk: the flush tail must be complete."""
    plan = male_plan(crate=20034.0)
    assert plan.info.control_steps == 1
    params = tracks.random_tracks(2, frames, seed0=4242, consonant_heavy=True)
    audio, counts, _ = plan.synthesize_host(params)
    cfg = oracle.male_config()
    for b in range(2):
        ref = oracle.synthesize(cfg, params[b], control_rate=20034.0)
        assert counts[b] == ref.size
        assert within(audio[b, : ref.size], ref, TOL_F64), peak_err(audio[b, : ref.size], ref)


# Over 1.2 M internal steps the last-bit differences between the device's and glibc's exp2/pow
# accumulate in the oscillator phase: measured 5e-9 of peak after 30 s.  The reference itself
# differs by 1.6e-8 between two builds of the same source, so 5e-8 is the fp64 bar here.
TOL_F64_LONG = 5e-8


@pytest.mark.parametrize("precision,tol", [(capi.PRECISION_F64, TOL_F64_LONG), (capi.PRECISION_MIXED, TOL_MIXED)], ids=["f64", "mixed"])
def test_long_form_oversampled_tube(precision, tol):
    """BASELINE.json configs[3] shape at reduced batch: 30 s tracks (7500 frames), 2x oversampled
    tube (VocalTractModel2<double,2> semantics, 40068 Hz internal).  Exact counts for all, two
    utterances checked against the oracle, the rest through determinism of the tiled batch."""
    pool = tracks.random_tracks(2, 7500, seed0=31337, consonant_heavy=True)
    params = np.concatenate([pool, pool, pool])  # 6 utterances, rows 0/2/4 and 1/3/5 identical
    plan = male_plan(delay=2, precision=precision)
    assert plan.info.internal_sample_rate == 40068 and plan.info.control_steps == 160
    audio, counts, maxabs = plan.synthesize_host(params)
    n = plan.output_count(7500)
    assert n == 1320787 and (counts == n).all()
    cfg = oracle.male_config(44100.0, 2)
    for b in range(2):
        ref = oracle.synthesize(cfg, pool[b])
        assert ref.size == n
        assert within(audio[b], ref, tol), peak_err(audio[b], ref)
        assert np.array_equal(audio[b], audio[b + 2]) and np.array_equal(audio[b], audio[b + 4])


def test_thirty_section_tube_batch_against_oracle():
    """VocalTractModel4 semantics (30 + 18 sections, one utterance per 48-lane tube wavefront),
    ragged batch, against the oracle."""
    frames = np.array([30, 0, 7, 30, 19], dtype=np.int32)
    params = tracks.random_tracks(len(frames), 30, seed0=440, consonant_heavy=True)
    plan = male_plan(layout=1)
    assert plan.info.internal_sample_rate == 60102
    audio, counts, _ = plan.synthesize_host(params, frames)
    cfg = oracle.male_config(44100.0, 1, 1)
    for b, f in enumerate(frames):
        ref = oracle.synthesize(cfg, params[b, :f]) if f else np.zeros(oracle.output_count(cfg, 0), np.float32)
        assert counts[b] == ref.size
        assert within(audio[b, : ref.size], ref, TOL_F64), peak_err(audio[b, : ref.size], ref)


@pytest.mark.parametrize("delay,layout", [(1, 0), (3, 0), (1, 1)])
def test_special_case_frames(delay, layout):
    """tracks.edge_track: volumes 0 / 60 dB, frication at the first / last section, radii at the floor, velum 0, pitch and
    band-pass extremes — fp64 path against the double oracle."""
    tr = tracks.edge_track(48)
    plan = male_plan(delay=delay, layout=layout)
    ref = oracle.synthesize(oracle.male_config(44100.0, delay, layout), tr)
    audio, counts, _ = plan.synthesize_host(np.stack([tr, tracks.random_track(48, 3, True), tr]))
    assert counts[0] == ref.size and np.isfinite(audio).all()
    assert within(audio[0, : ref.size], ref, TOL_F64), peak_err(audio[0, : ref.size], ref)
    assert np.array_equal(audio[2], audio[0])


@pytest.mark.parametrize("precision,rows", [(capi.PRECISION_F64, 2), (capi.PRECISION_MIXED, 4), (capi.PRECISION_MIXED, 2)], ids=["f64x2", "mixedx4", "mixedx2"])
def test_samples_do_not_depend_on_the_row_in_the_workgroup(precision, rows):
    """Several utterances per workgroup (the shape a big batch would get, forced through the diagnostics library): the same
    track must give the same samples, bit for bit, in whichever DPP row and workgroup it lands (the resampler's per-row
    code is unrolled)."""
    plan = male_plan(delay=2, precision=precision, rows=rows)
    pool = tracks.random_tracks(3, 60, seed0=8100, consonant_heavy=True)
    order = [0, 1, 2, 2, 0, 1, 1, 2, 0, 0, 0]  # every track in several rows and workgroups
    audio, counts, _ = plan.synthesize_host(pool[order])
    first = {t: order.index(t) for t in range(3)}
    for b, t in enumerate(order):
        assert np.array_equal(audio[b], audio[first[t]]), (b, t)
    alone, _, _ = male_plan(delay=2, precision=precision).synthesize_host(pool[:1])
    assert np.array_equal(alone[0], audio[0])  # and the same as one utterance per workgroup
