"""The packed host entries (gvtm_packed_sample_offsets, gvtm_synthesize_packed_host*, gvtm_plan_set_staging_limit,
gvtm_plan_packed_stats, gvtm_plan_reserve) on design-only plans.  No GPU needed.

Pins: the seven names in both libraries; the layout rule (exact counts, every start a multiple of 8) on the numbers the
CPU oracle gives for the male voice, over all eight residues of the count mod 8 on the female voice, and on a flush-overrun
length whose utterance is longer than its longer neighbour; every refusal of the tables, with its status and, for voice
ids, the utterance named; GVTM_ERR_NO_DEVICE after the argument checks; the limit and the stats without a device; and that
examples/synthesize_packed.c compiles as strict C99 and runs."""
import ctypes
import os

import numpy as np
import pytest

import gama_tts_amd as g
from gama_tts_amd import capi
import oracle
from voice_cases import configs, male_plan, oracle_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, NO_DEVICE = 0, 1, 2
BAD = ctypes.c_size_t(-1).value
NAMES = ["gvtm_packed_sample_offsets", "gvtm_synthesize_packed_host", "gvtm_synthesize_packed_host_pcm16",
         "gvtm_plan_set_staging_limit", "gvtm_plan_packed_stats", "gvtm_plan_reserve"]


def offsets_of(frame_counts):
    return np.concatenate([[0], np.cumsum(frame_counts)]).astype(np.int64)


def test_both_libraries_export_the_packed_entries():
    header = open(os.path.join(ROOT, "include", "gama_vtm.h")).read()
    assert "#define GVTM_PACKED_ALIGN 8" in header and "typedef struct gvtm_packed_stats" in header  # (the seventh name)
    assert capi.PACKED_ALIGN == 8
    for diagnostics in (False, True):
        lib = g.load_library(diagnostics)
        for name in NAMES:
            assert name in header and hasattr(lib, name), (name, diagnostics)


@pytest.mark.parametrize("precision", [capi.PRECISION_F64, capi.PRECISION_F32], ids=["f64", "f32"])
def test_layout_of_the_male_voice(precision):
    plan = male_plan(precision=precision, device=capi.DEVICE_NONE)
    frames = [0, 1, 8, 18]
    ocfg = oracle.male_config(44100.0, 1, float_model=1 if precision == capi.PRECISION_F32 else 0)
    assert [oracle.output_count(ocfg, f) for f in frames] == [58, 234, 1467, 3228]
    assert [plan.output_count(f) for f in frames] == [58, 234, 1467, 3228]
    off = plan.packed_sample_offsets(offsets_of(frames))
    assert off.tolist() == [0, 64, 304, 1776, 5008]
    # the return value is the capacity; the table itself may be left out
    fo = offsets_of(frames)
    assert plan._lib.gvtm_packed_sample_offsets(plan._h, fo.ctypes.data, None, 4, None) == 5008
    assert plan._lib.gvtm_packed_sample_offsets(plan._h, fo.ctypes.data, None, 0, None) == 0


def test_layout_covers_every_residue_of_the_count():
    vp = g.VoicesPlan(configs(names=["male", "female"]), 250.0, capi.DEVICE_NONE)
    frames = list(range(21))
    counts = [vp.voice_output_count(1, f) for f in frames]
    assert sorted(set(c % 8 for c in counts)) == list(range(8))  # what the rest of this test relies on
    ocfg = oracle_config("female", 44100.0, 1, 0, capi.PRECISION_F64)
    assert counts == [oracle.output_count(ocfg, f) for f in frames]
    off = vp.packed_sample_offsets(offsets_of(frames), np.ones(21, np.int32))
    assert off[0] == 0 and not (off % 8).any()
    for b, c in enumerate(counts):
        assert off[b + 1] == (off[b] + c + 7) // 8 * 8, b
    # the voice decides the count: the same frames under voice 0
    off0 = vp.packed_sample_offsets(offsets_of(frames), np.zeros(21, np.int32))
    assert np.array_equal(np.diff(off0), [(vp.voice_output_count(0, f) + 7) // 8 * 8 for f in frames])
    assert not np.array_equal(off0, off)


def test_extents_follow_the_counts_at_a_flush_overrun():
    plan = male_plan(rate=22050.0, delay=2, device=capi.DEVICE_NONE)
    assert plan.info.upsampling == 0
    assert (plan.output_count(18), plan.output_count(19)) == (2175, 1700)  # the shorter utterance is the longer one
    off = plan.packed_sample_offsets(offsets_of([19, 18, 3, 18, 0]))
    want = [0]
    for f in (19, 18, 3, 18, 0):
        want.append((want[-1] + plan.output_count(f) + 7) // 8 * 8)
    assert off.tolist() == want
    assert off[2] - off[1] == 2176 > off[1] - off[0] == 1704


def _call(plan, frames, fo, ids, out, capacity=None, pcm=False, batch=None):
    lib = plan._lib
    batch = len(fo) - 1 if batch is None else batch
    p = lambda x: None if x is None else x.ctypes.data  # noqa: E731
    capacity = (0 if out is None else out.size) if capacity is None else capacity
    if pcm:
        return lib.gvtm_synthesize_packed_host_pcm16(plan._h, p(frames), p(fo), p(ids), batch, p(out), capacity, None, None, None, None)
    return lib.gvtm_synthesize_packed_host(plan._h, p(frames), p(fo), p(ids), batch, p(out), capacity, None, None, None)


@pytest.mark.parametrize("pcm", [False, True], ids=["f32", "pcm16"])
def test_refusals_and_no_device(pcm):
    plan = male_plan(device=capi.DEVICE_NONE)
    lib = plan._lib
    fo = offsets_of([2, 0, 3])
    frames = np.zeros((5, 16), np.float32)
    cap = int(plan.packed_sample_offsets(fo)[-1])
    out = np.zeros(cap, np.int16 if pcm else np.float32)
    # a good call gets as far as the missing device
    assert _call(plan, frames, fo, None, out, pcm=pcm) == NO_DEVICE
    assert _call(plan, frames, fo, np.zeros(3, np.int32), out, pcm=pcm) == NO_DEVICE  # ids on a one-voice plan
    # nulls where something is due
    h = plan._h
    plan._h = None
    assert _call(plan, frames, fo, None, out, pcm=pcm) == INVALID
    plan._h = h
    assert _call(plan, frames, None, None, out, pcm=pcm, batch=3) == INVALID
    assert _call(plan, None, fo, None, out, pcm=pcm) == INVALID
    assert _call(plan, frames, fo, None, None, capacity=cap, pcm=pcm) == INVALID
    assert b"null" in lib.gvtm_last_error()
    # offsets that do not start at 0, offsets that decrease
    assert _call(plan, frames, fo + 1, None, out, pcm=pcm) == INVALID
    assert _call(plan, frames, np.array([0, 3, 2, 5], np.int64), None, out, pcm=pcm) == INVALID
    assert b"frame_offsets" in lib.gvtm_last_error()
    # voice ids outside [0, n_voices): the first such utterance is named
    assert _call(plan, frames, fo, np.array([0, 0, 1], np.int32), out, pcm=pcm) == INVALID
    assert b"utterance 2" in lib.gvtm_last_error()
    assert _call(plan, frames, fo, np.array([0, -1, 7], np.int32), out, pcm=pcm) == INVALID
    assert b"utterance 1" in lib.gvtm_last_error()
    # an utterance beyond the 31-bit step counter (the tables are judged before any frame is read)
    steps = plan.info.control_steps
    too_long = (1 << 31) // steps + 1
    assert _call(plan, frames, np.array([0, 2, 2 + too_long, 3 + too_long], np.int64), None, out, pcm=pcm) == INVALID
    assert b"31-bit" in lib.gvtm_last_error() and b"utterance 1" in lib.gvtm_last_error()
    # a capacity below the layout's
    assert _call(plan, frames, fo, None, out, capacity=cap - 1, pcm=pcm) == INVALID
    assert b"capacity" in lib.gvtm_last_error()


def test_layout_entry_refuses_what_the_synthesis_entries_refuse():
    plan = male_plan(device=capi.DEVICE_NONE)
    lib = plan._lib
    fo = offsets_of([2, 0, 3])
    out = np.full(4, -7, np.int64)
    assert lib.gvtm_packed_sample_offsets(None, fo.ctypes.data, None, 3, out.ctypes.data) == BAD
    assert lib.gvtm_packed_sample_offsets(plan._h, None, None, 3, out.ctypes.data) == BAD
    assert lib.gvtm_packed_sample_offsets(plan._h, (fo + 1).ctypes.data, None, 3, out.ctypes.data) == BAD
    dec = np.array([0, 3, 2, 5], np.int64)
    assert lib.gvtm_packed_sample_offsets(plan._h, dec.ctypes.data, None, 3, out.ctypes.data) == BAD
    ids = np.array([0, 4, 0], np.int32)
    assert lib.gvtm_packed_sample_offsets(plan._h, fo.ctypes.data, ids.ctypes.data, 3, out.ctypes.data) == BAD
    assert b"utterance 1" in lib.gvtm_last_error()
    assert (out == -7).all()  # a refused call writes nothing


def test_several_voices_need_ids():
    vp = g.VoicesPlan(configs(), 250.0, capi.DEVICE_NONE)
    fo = offsets_of([2, 0, 3])
    frames = np.zeros((5, 16), np.float32)
    ids = np.array([4, 0, 2], np.int32)
    cap = int(vp.packed_sample_offsets(fo, ids)[-1])
    out = np.zeros(cap, np.float32)
    assert vp._lib.gvtm_packed_sample_offsets(vp._h, fo.ctypes.data, None, 3, None) == BAD
    assert _call(vp, frames, fo, None, out) == INVALID
    assert b"voice" in vp._lib.gvtm_last_error()
    assert _call(vp, frames, fo, np.array([4, 5, 2], np.int32), out) == INVALID
    assert b"utterance 1" in vp._lib.gvtm_last_error()
    assert _call(vp, frames, fo, ids, out) == NO_DEVICE
    assert _call(vp, frames, fo, ids, out.view(np.int16), capacity=cap, pcm=True) == NO_DEVICE
    with pytest.raises(g.GvtmError) as err:
        vp.synthesize_packed_host([np.zeros((2, 16), np.float32)] * 3, ids)
    assert err.value.status == NO_DEVICE


def test_limit_stats_and_reserve_without_a_device():
    plan = male_plan(precision=capi.PRECISION_F32, device=capi.DEVICE_NONE)
    st = plan.packed_stats()
    assert (st.staging_bytes, st.limit, st.slices, st.largest_slice) == (0, 0, 0, 0)
    plan.set_staging_limit(3 << 20)
    assert plan.packed_stats().limit == 3 << 20 and plan.packed_stats().staging_bytes == 0
    plan.set_staging_limit(0)
    assert plan.packed_stats().limit == 0
    lib = plan._lib
    assert lib.gvtm_plan_reserve(plan._h, 20) == NO_DEVICE
    assert lib.gvtm_plan_reserve(None, 20) == INVALID
    assert lib.gvtm_plan_set_staging_limit(None, 1) == INVALID
    assert lib.gvtm_plan_packed_stats(plan._h, None) == INVALID and lib.gvtm_plan_packed_stats(None, ctypes.byref(st)) == INVALID


def test_packed_example_builds_and_runs(tmp_path):
    """examples/synthesize_packed.c: three utterances of 40, 250 and 7 frames; the layout without a device, the int16
    samples with one."""
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    inc = os.path.join(ROOT, "include")
    libdir = os.path.dirname(g.library_path())
    exe = str(tmp_path / "synthesize_packed")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-O1", "-I" + inc, os.path.join(ROOT, "examples", "synthesize_packed.c"),
                    "-L" + libdir, "-lgama_vtm", "-Wl,-rpath," + libdir, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr)
    plan = male_plan(device=capi.DEVICE_NONE)
    off = plan.packed_sample_offsets(offsets_of([40, 250, 7]))
    for b, f in enumerate((40, 250, 7)):
        assert "utterance %d: %d frames -> %d samples at offset %d" % (b, f, plan.output_count(f), off[b]) in r.stdout
    assert "packed output: %d samples" % off[3] in r.stdout
    if g.device_count() == 0:
        assert "no HIP device" in r.stdout
    else:
        assert "utterance 1: %d samples at [%d, %d)" % (plan.output_count(250), off[1], off[1] + plan.output_count(250)) in r.stdout
