"""Event lists in from host memory, packed samples out (gvtm_events_packed_layout, gvtm_synthesize_events_packed_host*) on
design-only plans.  No GPU needed.

Pins: the three names in both libraries and the kernel hook in the diagnostics library alone; the layout (frames per
utterance = gvtm_tracks_chunks_frame_count, sample offsets = gvtm_packed_sample_offsets of their prefix sum) for utterances
of 0 to 3 chunks with empty and one-event chunks among them, on a one-voice plan and on a five-voice plan with interleaved
ids; every refusal in the header's order, one case each, with outputs pre-filled with sentinels that must come back
untouched; GVTM_ERR_NO_DEVICE after the checks; batch == 0; and that examples/synthesize_events.c compiles as strict C99
and runs."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import gama_tts_amd as g
from gama_tts_amd import capi
import event_lists

from chunk_cases import list_with_frames, offset_tables
from voice_cases import configs, male_plan, model5_plan, track_configs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, NO_DEVICE = 0, 1, 2
BAD = ctypes.c_size_t(-1).value
NAMES = {"gvtm_events_packed_layout", "gvtm_synthesize_events_packed_host", "gvtm_synthesize_events_packed_host_pcm16"}
HOOK = "gvtm_debug_tracks_slice"


def exported(diagnostics=False):
    out = subprocess.run(["nm", "-D", "--defined-only", capi.library_path(diagnostics)], check=True, capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.split()}


def test_names_and_the_hook():
    header = open(os.path.join(ROOT, "include", "gama_vtm.h")).read()
    for name in NAMES:
        assert name + "(" in header
    assert HOOK not in header
    assert "Controller::synthesizePhoneticStringToFile" in header and "Controller.cpp:194-200" in header
    assert "round_up(296 * events_of_slice, 64)" in header
    assert NAMES <= exported() and NAMES <= exported(diagnostics=True)
    assert HOOK in exported(diagnostics=True) and HOOK not in exported()


def per_frame_count(control_period, times):
    """the control-period loop of EventList::generateOutput (EventList.cpp:985-1032), frame by frame"""
    if len(times) < 2:
        return 0
    target, n, now = 1, 0, 0
    while True:
        n += 1
        now += control_period
        if now >= times[target]:
            target += 1
            if target == len(times):
                return n


def test_the_hosts_walk_counts_what_the_per_frame_loop_counts():
    """The layout is built on gvtm_tracks_frame_count, which steps from event to event: on and off the control-period grid,
    several events inside one period, events that share a time, every control period."""
    for cp in (1, 2, 3, 4):
        cfg = track_configs(["male"])[0]
        cfg.control_period_ms = cp
        for seed in range(24):
            for min_gap in (None, 0, 1, 3):
                t = event_lists.random_event_table(seed, n_events=seed, control_period=cp, min_gap_ms=min_gap)
                assert capi.tracks_frame_count(cfg, capi.events_from_table(t)) == per_frame_count(cp, [int(x) for x in t[:, 0]]), (cp, seed, min_gap)


def male_tracks_plan(**kw):
    plan = male_plan(device=capi.DEVICE_NONE, **kw)
    plan.set_voice_tracks(track_configs(["male"]))
    return plan


def ragged_utterances():
    """Utterances of 0, 1, 2 and 3 chunks; empty and one-event chunks in front, in the middle and alone."""
    L = lambda seed, n: event_lists.random_event_table(seed, n_events=n)  # noqa: E731
    e0, e1 = L(50, 0), L(51, 1)
    return [[], [L(1, 40)], [L(2, 17), L(3, 33)], [e0, e1, list_with_frames(33)], [e1], [list_with_frames(1), e0, L(4, 9)], [e0]]


def expected_layout(plan, utterances, ids, track_cfgs):
    frames = []
    for b, u in enumerate(utterances):
        events, chunk_offsets, _ = offset_tables([u])
        frames.append(capi.tracks_chunks_frame_count(track_cfgs[0 if ids is None else ids[b]], events, chunk_offsets))
    frame_offsets = np.concatenate([[0], np.cumsum(frames)]).astype(np.int64)
    return frame_offsets, plan.packed_sample_offsets(frame_offsets, ids)


def test_layout_of_a_one_voice_plan():
    plan = male_tracks_plan()
    utterances = ragged_utterances()
    events, chunk_offsets, utt_chunks = plan.pack_event_lists(utterances)
    assert np.diff(utt_chunks).tolist() == [0, 1, 2, 3, 1, 3, 1]
    frame_offsets, sample_offsets = plan.events_packed_layout(events, chunk_offsets, utt_chunks)
    want_frames, want_samples = expected_layout(plan, utterances, None, track_configs(["male"]))
    assert np.array_equal(frame_offsets, want_frames) and np.array_equal(sample_offsets, want_samples)
    counts = np.diff(frame_offsets)
    assert counts[0] == counts[4] == counts[6] == 0 and counts[3] == 33 and (counts[[1, 2, 5]] > 1).all()
    # the return value is the capacity; either table may be left out; ids of zeros on a one-voice plan change nothing
    p = lambda x: x.ctypes.data  # noqa: E731
    assert plan._lib.gvtm_events_packed_layout(plan._h, p(events), p(chunk_offsets), p(utt_chunks), None, 7, None, None) == sample_offsets[7]
    assert np.array_equal(plan.events_packed_layout(events, chunk_offsets, utt_chunks, np.zeros(7, np.int32))[1], sample_offsets)
    assert plan._lib.gvtm_events_packed_layout(plan._h, None, None, None, None, 0, None, None) == 0


def test_layout_of_five_voices_interleaved():
    plan = g.VoicesPlan(configs(), 250.0, capi.DEVICE_NONE)
    plan.set_voice_tracks(track_configs())
    utterances = ragged_utterances() * 2
    ids = (np.arange(len(utterances)) % 5).astype(np.int32)
    events, chunk_offsets, utt_chunks = plan.pack_event_lists(utterances)
    frame_offsets, sample_offsets = plan.events_packed_layout(events, chunk_offsets, utt_chunks, ids)
    want_frames, want_samples = expected_layout(plan, utterances, ids, track_configs())
    assert np.array_equal(frame_offsets, want_frames) and np.array_equal(sample_offsets, want_samples)
    # the same lists give the same frames under every voice and another sample count: utterances 1 and 8 (voices 1 and 3)
    assert np.diff(frame_offsets)[1] == np.diff(frame_offsets)[8] and np.diff(sample_offsets)[1] != np.diff(sample_offsets)[8]
    # several voices need ids
    p = lambda x: x.ctypes.data  # noqa: E731
    assert plan._lib.gvtm_events_packed_layout(plan._h, p(events), p(chunk_offsets), p(utt_chunks), None, len(utterances), None, None) == BAD
    assert b"voice" in plan._lib.gvtm_last_error()


class Call:
    """One call of the float32 or the int16 entry on a small good batch, every argument replaceable, every output array
    pre-filled with a sentinel."""

    def __init__(self, plan, pcm, frames_out=True):
        self.plan, self.pcm = plan, pcm
        self.events, self.chunk_offsets, self.utt_chunks = plan.pack_event_lists([[list_with_frames(3)], [], [list_with_frames(2), list_with_frames(1)]])
        self.frame_offsets, self.sample_offsets = plan.events_packed_layout(self.events, self.chunk_offsets, self.utt_chunks)
        assert self.frame_offsets.tolist() == [0, 3, 3, 6]
        self.capacity = int(self.sample_offsets[-1])
        self.out = dict(audio=np.full(self.capacity, 12345 if pcm else 7.0, np.int16 if pcm else np.float32),
                        sample_offsets=np.full(4, -7, np.int64), frame_offsets=np.full(4, -7, np.int64),
                        frames=np.full((6, 16), 7.0, np.float32) if frames_out else None, counts=np.full(3, -7, np.int64),
                        maxabs=np.full(3, -7.0, np.float32), scales=np.full(3, -7.0, np.float32), drift=np.full((3, 5), 0.25, np.float64))
        self.before = {k: None if v is None else v.copy() for k, v in self.out.items()}

    def __call__(self, **replace):
        o = self.out
        a = dict(plan=self.plan._h, events=self.events, chunk_offsets=self.chunk_offsets, utt_chunks=self.utt_chunks, ids=None, batch=3,
                 audio=o["audio"], capacity=self.capacity, frames=o["frames"], frames_capacity=6)
        a.update(replace)
        p = lambda x: x.ctypes.data if isinstance(x, np.ndarray) else x  # noqa: E731
        lib = self.plan._lib
        head = (p(a["plan"]), p(a["events"]), p(a["chunk_offsets"]), p(a["utt_chunks"]), p(a["ids"]), a["batch"], p(a["audio"]), a["capacity"],
                p(o["sample_offsets"]), p(o["frame_offsets"]), p(a["frames"]), a["frames_capacity"], p(o["counts"]), p(o["maxabs"]))
        if self.pcm:
            rc = lib.gvtm_synthesize_events_packed_host_pcm16(*head, p(o["scales"]), p(o["drift"]))
        else:
            rc = lib.gvtm_synthesize_events_packed_host(*head, p(o["drift"]))
        for k, v in self.out.items():  # a refused call writes nothing
            assert v is None or np.array_equal(v, self.before[k]), k
        return rc


@pytest.mark.parametrize("pcm", [False, True], ids=["f32", "pcm16"])
def test_refusals_in_order_and_no_device(pcm):
    plan = male_tracks_plan()
    call = Call(plan, pcm)
    error = lambda: plan._lib.gvtm_last_error().decode()  # noqa: E731
    # a good call gets as far as the missing device, with or without ids, frames and drift
    assert call() == NO_DEVICE and "design-only" in error()
    assert call(ids=np.zeros(3, np.int32)) == NO_DEVICE
    assert call(frames=None, frames_capacity=0) == NO_DEVICE
    # 1. a null plan (everything else wrong too: the first check wins)
    assert call(plan=None, chunk_offsets=None, audio=None) == INVALID and "null plan" in error()
    # 2. a plan without track configurations
    bare = male_plan(device=capi.DEVICE_NONE)
    assert call(plan=bare._h, chunk_offsets=None) == INVALID and "gvtm_plan_set_voice_tracks" in error()
    # 3. a null table
    assert call(chunk_offsets=None, events=None) == INVALID and "null chunk_offsets or utt_chunks" in error()
    assert call(utt_chunks=None, events=None) == INVALID and "null chunk_offsets or utt_chunks" in error()
    # 4. null events while chunks are present (in front of the tables' order)
    assert call(events=None, utt_chunks=np.array([0, 2, 1, 3], np.int64)) == INVALID and "null events" in error()
    # 5. tables that do not start at 0, or that decrease
    assert call(utt_chunks=np.array([1, 1, 1, 3], np.int64), ids=np.full(3, 9, np.int32)) == INVALID and "utt_chunks" in error()
    assert call(utt_chunks=np.array([0, 2, 1, 3], np.int64)) == INVALID and "utt_chunks" in error()
    assert call(chunk_offsets=call.chunk_offsets + 1) == INVALID and "chunk_offsets" in error()
    assert call(chunk_offsets=np.array([0, 4, 3, 6], np.int64)) == INVALID and "chunk_offsets" in error()
    # 6. the ids, as the packed entry checks them: the first bad utterance is named
    assert call(ids=np.array([0, 0, 1], np.int32), audio=None) == INVALID and "utterance 2" in error()
    assert call(ids=np.array([0, -1, 7], np.int32)) == INVALID and "utterance 1" in error()
    # 7. an utterance whose steps do not fit the 31-bit counter: one list whose last event lies 2^31 / steps periods out
    too_long = (1 << 31) // plan.info.control_steps + 1
    t = list_with_frames(2)
    t[-1, 0] = 4 * too_long
    events, chunk_offsets, utt_chunks = plan.pack_event_lists([[list_with_frames(3)], [t], []])
    assert 4 * too_long < 2 ** 31
    assert call(events=events, chunk_offsets=chunk_offsets, utt_chunks=utt_chunks, audio=None) == INVALID
    assert "31-bit" in error() and "utterance 1" in error()
    # 8. a null output buffer where one is due
    assert call(audio=None, capacity=0) == INVALID and ("null pcm buffer" if pcm else "null audio buffer") in error()
    # 9. a capacity below the layout's: the samples', and the frames' when frames are asked for
    assert call(capacity=call.capacity - 1) == INVALID and "capacity" in error()
    assert call(frames_capacity=5) == INVALID and "frames_capacity" in error()
    assert call(frames=None, frames_capacity=0) == NO_DEVICE
    # 10. a design-only plan, after all of these; 11. batch == 0 on it too
    assert call(batch=0) == NO_DEVICE


def test_layout_entry_refuses_what_the_synthesis_entries_refuse():
    plan = male_tracks_plan()
    call = Call(plan, False)
    lib = plan._lib
    fo, so = np.full(4, -7, np.int64), np.full(4, -7, np.int64)
    p = lambda x: None if x is None else x.ctypes.data  # noqa: E731

    def layout(h=plan._h, events=call.events, chunk_offsets=call.chunk_offsets, utt_chunks=call.utt_chunks, ids=None):
        return lib.gvtm_events_packed_layout(h, p(events), p(chunk_offsets), p(utt_chunks), p(ids), 3, p(fo), p(so))

    assert layout() == call.capacity and np.array_equal(fo, call.frame_offsets) and np.array_equal(so, call.sample_offsets)
    fo[:], so[:] = -7, -7
    assert layout(h=None) == BAD
    assert layout(h=male_plan(device=capi.DEVICE_NONE)._h) == BAD
    assert layout(chunk_offsets=None) == BAD and layout(utt_chunks=None) == BAD and layout(events=None) == BAD
    assert layout(utt_chunks=np.array([0, 2, 1, 3], np.int64)) == BAD and layout(chunk_offsets=call.chunk_offsets + 1) == BAD
    assert layout(ids=np.array([0, 4, 0], np.int32)) == BAD and b"utterance 1" in lib.gvtm_last_error()
    assert (fo == -7).all() and (so == -7).all()  # a refused call writes nothing


def test_model5_float_plan_and_batch_zero():
    plan = model5_plan("male", float_class=True, device=capi.DEVICE_NONE)
    plan.set_voice_tracks(track_configs(["male"], model5=True))
    call = Call(plan, True, frames_out=False)
    assert call(frames=None, frames_capacity=0) == NO_DEVICE
    # batch == 0 needs no table and no buffer: NO_DEVICE here, GVTM_OK where there is a device
    assert call(batch=0, events=None, chunk_offsets=None, utt_chunks=None, audio=None, capacity=0, frames=None, frames_capacity=0) == NO_DEVICE


def test_events_example_builds_and_runs(tmp_path):
    """examples/synthesize_events.c: utterances of one, two and no chunks; the layout without a device, the int16 samples
    and the frames with one."""
    import shutil
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    inc = os.path.join(ROOT, "include")
    libdir = os.path.dirname(g.library_path())
    exe = str(tmp_path / "synthesize_events")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-O1", "-I" + inc, os.path.join(ROOT, "examples", "synthesize_events.c"),
                    "-L" + libdir, "-lgama_vtm", "-Wl,-rpath," + libdir, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr)
    plan = male_tracks_plan()
    off = plan.packed_sample_offsets(np.array([0, 100, 180, 180], np.int64))  # 400 ms, 200 + 120 ms and nothing at 4 ms per frame
    for b, (chunks, frames) in enumerate(((1, 100), (2, 80), (0, 0))):
        assert "utterance %d: %d chunks -> %d frames -> samples at offset %d" % (b, chunks, frames, off[b]) in r.stdout
    assert "packed output: %d samples, 180 frames" % off[3] in r.stdout
    if g.device_count() == 0:
        assert "no HIP device" in r.stdout
    else:
        assert "utterance 1: %d samples at [%d, %d)" % (plan.output_count(80), off[1], off[1] + plan.output_count(80)) in r.stdout
