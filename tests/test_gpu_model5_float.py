"""The float class of reference model 5 on the GPU (gvtm_plan_create_model5_float: VocalTractModel5<float,1>, the kernel of
csrc/vtm_kernels_m5f.hip).

The bar is bit identity -- parity_rules.within(got, ref, TOL[PRECISION_F32]) -- with sample counts exact and
maxabs == abs(out).max(): every LDS record, recurrence and the tube are float, every rounding of the class is reproduced,
so nothing is left to tolerate.  References are the committed vectors of the real class (tests/golden/vtm5_golden.npz's three
"5f" cases, seeds 31 and 32 of random_golden.npz, tests/golden/vtm5f_golden.npz) and the float oracle, which
tests/test_oracle5_vs_golden.py and tests/test_oracle5f_vs_golden.py hold to those vectors.

The class has two workgroup shapes (vtm_kernel_m5.inc: chunk 60 up to 256 utterances, chunk 56 -- two workgroups per
compute unit -- beyond); a diagnostics plan forces either (rows 1 / rows 2), and both must give the same bits."""
import ctypes
import functools
import hashlib
import os

import numpy as np
import pytest

import gama_tts_amd as g
from gama_tts_amd import capi
import golden_cases
import model5_cases as cases
import oracle
import tracks
import voice_files
from device_io import events_chain_and_entry
from parity_rules import TOL, check_batch, within
from track_cases import product_config, singable_event_table, used_drift
from voice_cases import model5_plan, push_in_pieces

pytestmark = pytest.mark.gpu

BIT_IDENTICAL = TOL[capi.PRECISION_F32]
LIBDIR = os.path.dirname(g.library_path())
PLUGIN = os.path.join(LIBDIR, "libgama_vtm_plugin.so")


# float5_plan(overrides, rate, crate, rows): a float model-5 plan of the 5_male voice on device 0 (rows 1 / 2: a diagnostics
# plan forced to chunk 60 / chunk 56)
float5_plan = functools.partial(model5_plan, "male", float_class=True)


@pytest.mark.parametrize("rows", [0, 2], ids=["product_shape", "chunk56"])
@pytest.mark.parametrize("case", cases.MALE_FLOAT_CASES, ids=lambda c: c["name"])
def test_reference_vectors(case, rows, golden):
    data = cases.load(case["fixture"])
    m = data["manifest"][case["name"]]
    tr = cases.track_for(case, golden)
    plan = float5_plan(case["overrides"], case["rate"], case["crate"], rows)
    assert plan.info.model5 == 1 and plan.info.precision == capi.PRECISION_F32
    assert plan.info.control_steps * tr.shape[0] == m["steps"]
    audio, counts, maxabs = plan.synthesize_host(tr[None])
    assert counts[0] == m["n"] == plan.output_count(tr.shape[0])
    out = audio[0, : m["n"]]
    assert hashlib.sha256(out.tobytes()).hexdigest() == m["sha256"]
    for got, key in cases.stored(case, out):
        assert within(got, data[key], BIT_IDENTICAL), key
    assert maxabs[0] == np.abs(out).max() == np.float32(m["maxabs"])


@pytest.mark.parametrize("seed", [31, 32])
def test_random_vectors_of_the_reference_binary(seed):
    tr = tracks.random_track(60, seed, seed % 2 == 0)
    audio, counts, maxabs = float5_plan().synthesize_host(tr[None])
    m = golden_cases.check_against_random_golden(audio[0, : counts[0]], "5f", seed)
    assert maxabs[0] == np.abs(audio[0, : m["n"]]).max()


def test_ragged_batch_with_the_flush_overrun_against_the_float_oracle():
    frames = [0, 1, 2, 3, 7, 25, 40, 40, 13, 31, 106]
    params = tracks.random_tracks(len(frames), 106, seed0=900, consonant_heavy=True)
    cfg = oracle.male5_config(44100.0, 1)
    refs = [oracle.synthesize5(cfg, params[b, :f])[0] for b, f in enumerate(frames)]
    assert refs[10].size > oracle.synthesize5(cfg, np.zeros((107, 16), np.float32))[0].size  # (106 frames: the overrun)
    for rows in (0, 2):
        audio, counts, maxabs = float5_plan(rate=44100.0, rows=rows).synthesize_host(params, frame_counts=frames)
        check_batch(audio, counts, maxabs, refs, True)


def test_upsampling_branch():
    tr = tracks.random_track(30, 5, True)
    plan = float5_plan(rate=96000.0)
    assert plan.info.upsampling == 1
    audio, counts, maxabs = plan.synthesize_host(tr[None])
    check_batch(audio, counts, maxabs, [oracle.synthesize5(oracle.male5_config(96000.0, 1), tr)[0]], True)


def test_special_case_frames():
    """tracks.edge_track (volumes 0 / 60 dB, frication at the first / last section incl. the dropped right share, radii
    at the floor, velum 0, pitch and band-pass extremes), alone and inside a batch."""
    tr = tracks.edge_track(48)
    other = tracks.random_track(48, 3, True)
    cfg = oracle.male5_config(48000.0, 1)
    ref, ref_other = oracle.synthesize5(cfg, tr)[0], oracle.synthesize5(cfg, other)[0]
    assert np.isfinite(ref).all()
    plan = float5_plan()
    check_batch(*plan.synthesize_host(tr[None]), [ref], True)
    check_batch(*plan.synthesize_host(np.stack([tr, other, tr])), [ref, ref_other, ref], True)


def test_long_utterance_next_to_short_ones():
    """600 frames (145 200 steps: the 16.16 time register wraps every 271 frames, the 1024-sample ring every 1024 steps) in
    one launch with a one-frame and an empty utterance."""
    long_tr = tracks.random_track(600, 11, True)
    params = np.zeros((3, 600, 16), np.float32)
    params[0] = long_tr
    params[1, :1] = long_tr[:1]
    cfg = oracle.male5_config(48000.0, 1)
    refs = [oracle.synthesize5(cfg, params[b, :f])[0] for b, f in enumerate((600, 1, 0))]
    check_batch(*float5_plan().synthesize_host(params, frame_counts=[600, 1, 0]), refs, True)


def test_product_library_on_a_batch_beyond_two_workgroups_per_compute_unit():
    """601 utterances (more than two per compute unit: the chunk-56 shape, sliced by the host entry) through libgama_vtm.so
    with nothing forced: a pool of 12 ragged tracks tiled, every pool member against the oracle, every copy equal to its
    first occurrence."""
    pool_f = np.array([30, 0, 7, 30, 19, 1, 30, 12, 25, 30, 3, 28], dtype=np.int32)
    pool = tracks.random_tracks(len(pool_f), 30, seed0=6000, consonant_heavy=True)
    batch = 601
    idx = np.arange(batch) % len(pool_f)
    audio, counts, maxabs = float5_plan().synthesize_host(pool[idx], pool_f[idx])
    cfg = oracle.male5_config(48000.0, 1)
    check_batch(audio, counts, maxabs, [oracle.synthesize5(cfg, pool[t, : pool_f[t]])[0] for t in range(len(pool_f))], True)
    for b in range(len(pool_f), batch):
        assert counts[b] == counts[b % len(pool_f)] and np.array_equal(audio[b], audio[b % len(pool_f)]), b
        assert maxabs[b] == maxabs[b % len(pool_f)]


@pytest.mark.parametrize("total", [[33, 33, 33], [33, 20, 8]], ids=["lockstep", "ragged"])
def test_stream_pieces_equal_the_one_shot_samples(total):
    total = np.array(total, dtype=np.int32)
    batch = tracks.random_tracks(3, 33, seed0=5700, consonant_heavy=True)
    plan = float5_plan()
    one, c1, m1 = plan.synthesize_host(batch, total)
    got, maxabs = push_in_pieces(plan, batch, total, (7, 1, 25))
    for b in range(3):
        assert got[b].size == c1[b] and np.array_equal(got[b], one[b, : c1[b]]), b
        assert maxabs[b] == m1[b]
    ref, _ = oracle.synthesize5(oracle.male5_config(48000.0, 1), batch[1, : total[1]])
    assert within(got[1], ref, BIT_IDENTICAL)


def test_stream_finish_on_a_flush_overrun():
    """106 frames at 44.1 kHz: finish converts the extra lap of the ring, as the one-shot launch does."""
    track = tracks.random_track(106, 5500, True)
    plan = float5_plan(rate=44100.0)
    whole, counts, peak = plan.synthesize_host(track[None])
    got, maxabs = push_in_pieces(plan, track[None], np.array([106], dtype=np.int32), (7, 1, 25, 73))
    assert got[0].size == counts[0] == plan.output_count(106) > plan.output_count(107)
    assert np.array_equal(got[0], whole[0, : counts[0]]) and maxabs[0] == peak[0]
    assert within(got[0], oracle.synthesize5(oracle.male5_config(44100.0, 1), track)[0], BIT_IDENTICAL)


def test_events_entry_equals_tracks_followed_by_synthesis():
    import torch
    cfgv = np.array([4, 1, 1, 1, 1, -20.0, -6.0, 4.0, 250.0, 4.0])
    pool_n = [40, 2, 1, 17, 60, 3, 55]
    tables = [singable_event_table(300 + b, n) for b, n in enumerate(pool_n)]
    tc = product_config(cfgv)
    frames_of = [capi.tracks_frame_count(tc, capi.events_from_table(t)) for t in tables]
    max_frames = max(frames_of)
    plan = float5_plan()
    stride = plan.output_capacity(max_frames)
    chain, entry, d_params = events_chain_and_entry(plan, tc, tables, max_frames, stride, used_drift(len(tables)))
    a1, f1, n1, m1, dr1 = chain
    a2, f2, n2, m2, dr2 = entry
    ok = torch.isfinite(a1).all(dim=1) & torch.isfinite(m1)
    assert bool(ok[0]) and int(ok.sum().item()) >= (len(tables) * 2) // 3
    assert torch.equal(f1, f2) and torch.equal(n1, n2) and f2.cpu().tolist() == frames_of
    assert torch.equal(dr1.view(torch.int64), dr2.view(torch.int64))
    assert torch.equal(m1[ok].view(torch.int32), m2[ok].view(torch.int32))
    assert torch.equal(a1[ok].view(torch.int32), a2[ok].view(torch.int32))
    frames0 = d_params[0, : frames_of[0]].cpu().numpy()
    ref, _ = oracle.synthesize5(oracle.male5_config(48000.0, 1), frames0)
    assert n2[0].item() == ref.size and within(a2[0, : ref.size].cpu().numpy(), ref, BIT_IDENTICAL)


def test_plugin_with_gpu_model_5_and_gpu_precision_f32_through_the_loaders(golden, golden5, tmp_path):
    """`gpu_model = 5` with `gpu_precision = f32` makes the plugin stand in for VocalTractModel5<float,1>: driven by
    oracle/_build/vtm_plugin_host and, where oracle/_ref/ref_vtm is present, by the reference's own loader."""
    keys = oracle.read_config_file(oracle.VOICE5_MALE)
    keys["gpu_model"] = "5"
    keys["gpu_precision"] = "f32"
    cfg = str(tmp_path / "vtm5f.txt")
    with open(cfg, "w") as f:
        for k, v in keys.items():
            f.write("%s = %s\n" % (k, v))
    tr = cases.track_for(cases.by_name("rand5_m5f"), golden)
    out, info = oracle.plugin_synthesize(tr, PLUGIN, tmpdir=str(tmp_path), output_rate=48000, config=cfg)
    if oracle.ref_binary() is not None:
        ref_out, _ = oracle.ref_synthesize(tr, "2000:" + PLUGIN, tmpdir=str(tmp_path), output_rate=48000, config=cfg)
        assert np.array_equal(out, ref_out)
    ref = golden5["rand5_m5f__out"]
    assert out.size == ref.size == int(info["N"])
    assert abs(float(info["fs"]) - golden5["manifest"]["rand5_m5f"]["fs"]) < 2e-3
    assert within(out, ref, BIT_IDENTICAL)
    assert within(out, oracle.synthesize5(oracle.male5_config(48000.0, 1), tr)[0], BIT_IDENTICAL)


def test_several_voices_entries_refuse_the_float_plan():
    """A float model-5 plan holds one voice and has no voice variant of its kernel: GVTM_ERR_UNSUPPORTED, nothing written."""
    plan = float5_plan()
    lib = g.load_library()
    params = np.zeros((2, 3, 16), np.float32)
    ids = np.zeros(2, np.int32)
    stride = plan.output_capacity(3)
    audio, counts, maxabs = np.full((2, stride), 7.0, np.float32), np.zeros(2, np.int64), np.zeros(2, np.float32)
    rc = lib.gvtm_synthesize_voices_host(plan._h, params.ctypes.data, None, ids.ctypes.data, 2, 3, audio.ctypes.data, stride,
                                         counts.ctypes.data, maxabs.ctypes.data)
    assert rc == 4 and (audio == 7.0).all()


def test_device_sinf_matches_libm_bit_for_bit():
    """sinf_glibc evaluated BY THE DEVICE against this machine's sinf over [0, 2 pi], the range of t * 2 pi of the sine
    waveform (RosenbergBGlottalSource.h:139), its ends and the identity range below 2^-12 included; the cosine and tangent
    arguments of model 5 stay inside the ranges tests/test_gpu_parity_f32.py probes (test_capi_model5_float_cpu.py)."""
    plan = float5_plan(rows=1)
    lib = g.load_library(diagnostics=True)
    rng = np.random.default_rng(5)
    f32 = np.float32
    x = np.concatenate([rng.uniform(0.0, 2 * np.pi, 500000), np.exp(rng.uniform(np.log(2.0 ** -14), np.log(0.8), 100000)),
                        [0.0, 2.0 ** -13, 2.0 ** -12, np.pi / 4, np.pi / 2, np.pi, 1.5 * np.pi]]).astype(f32)
    x = np.concatenate([x, [f32(1.0) * f32(2.0 * np.pi)]]).astype(f32)
    out = np.empty_like(x)
    assert lib.gvtm_debug_device_float_math(plan._h, 5, x.ctypes.data, x.size, out.ctypes.data) == 0
    libm = ctypes.CDLL("libm.so.6")
    libm.sinf.restype = ctypes.c_float
    libm.sinf.argtypes = [ctypes.c_float]
    # the host restatement equals libm on EVERY float of the range (test_capi_model5_float_cpu.py): the device against it,
    # and a sample of libm itself
    host = np.empty(x.size, np.float64)
    assert lib.gvtm_debug_short_math(8, x.astype(np.float64).ctypes.data, x.size, host.ctypes.data) == 0
    assert np.array_equal(out.view(np.uint32), host.astype(f32).view(np.uint32))
    for i in range(0, x.size, 997):
        assert out[i] == f32(libm.sinf(float(x[i]))), x[i]


def test_batched_vtm_cli_with_f_on_a_model5_voice(golden, tmp_path):
    """`gama_vtm_batch -f` on a voice whose vtm.txt says `model = 5` synthesizes with VocalTractModel5<float,1>: the WAV
    holds the float oracle's samples, scaled and rounded as Controller::writeOutputToFile does."""
    import struct
    import subprocess
    voice = str(tmp_path / "voice5")
    voice_files.write_voice_dir(voice, oracle.read_config_file(oracle.VOICE5_MALE), voice_files.VARIANT_KEYS5)
    out_dir = str(tmp_path / "out5f")
    os.makedirs(out_dir)
    tr = np.asarray(golden["hello_params"])[:40]
    path = str(tmp_path / "short5f.txt")
    with open(path, "w") as f:
        for row in tr:
            f.write(" ".join("%.9g" % v for v in row) + "\n")
    r = subprocess.run([os.path.join(LIBDIR, "gama_vtm_batch"), "-f", voice, out_dir, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    data = open(os.path.join(out_dir, "short5f.wav"), "rb").read()
    assert data[:4] == b"RIFF" and data[8:16] == b"WAVEfmt " and data[36:40] == b"data"
    assert struct.unpack("<IHHIIHH", data[16:36]) == (16, 1, 1, 48000, 96000, 2, 16)
    pcm = np.frombuffer(data[44:44 + struct.unpack("<I", data[40:44])[0]], dtype="<i2").astype(np.int32)

    def samples16(ref):
        scaled = (ref * np.float32(oracle.output_scale(ref))) * np.float32(32767.0)
        return (np.sign(scaled) * np.floor(np.abs(scaled) + np.float32(0.5))).astype(np.int32)

    want = samples16(oracle.synthesize5(oracle.male5_config(48000.0, 1), tr)[0])
    assert pcm.size == want.size
    # (the device samples are the float class's bit for bit; the 16-bit rounding of a sample on a .5 boundary may differ
    # by one step between the device's and numpy's scaling, as in tests/test_gpu_dropin.py)
    assert np.abs(pcm - want).max() <= 1 and np.mean(pcm == want) > 0.999
    # and they are not the double class's: the two classes drift apart by more than a 16-bit step
    other = samples16(oracle.synthesize5(oracle.male5_config(48000.0, 0), tr)[0])
    assert np.mean(pcm == want) > np.mean(pcm == other)
