"""GPU-box: rhythm and intonation points on the device (gvtm_synthesize_prosody_device) beside the route a
caller had before.

4096 utterances of the 54-posture sentence of tests/golden/prosody_golden.npz (sentence.0: 11 feet, one tone group, 37 rule
applications, 13 points), each under draws of its own, float plan of the male voice with macro intonation, control period 4 ms:
  new     gvtm_synthesize_prosody_device on the postures before rhythm
  today   gvtm_generate_events_device on the postures after rhythm; rule data, rule counts, onsets and statuses copied to
          page-locked memory; synchronise; gvtm_prosody_points_host per utterance on one host core (the C entry through
          prebuilt ctypes arguments); points and offsets copied back; gvtm_synthesize_intonation_device
Both start from tables that lie on the device.  `today` is also timed in its parts: the device work in front of the
synchronisation, the host loop, and an empty loop of as many ctypes calls (what the binding, not the rule, costs).
Before anything is timed the two routes' samples, counts, peaks and statuses are compared byte for byte.  The routes
alternate inside every repeat; medians of a host clock around work that ends in a device synchronise.
usage: python tests/tools/bench_prosody.py [--reps N] [--batch B] [--kernels] [--out FILE.json]"""
import argparse
import ctypes
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import gama_tts_amd as g  # noqa: E402
from gama_tts_amd import capi  # noqa: E402
import oracle  # noqa: E402
import prosody_cases as cases  # noqa: E402
import rules_cases  # noqa: E402

ENTRY = "sentence.0"
MAX_RULES = 40


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    batch = args.batch
    stream = torch.cuda.current_stream().cuda_stream
    golden = np.load(cases.GOLDEN)
    lib = capi.load_library()
    rules = capi.Rules(dict(np.load(rules_cases.MODEL_0_MALE)), device=0)
    prosody = capi.Prosody(capi.prosody_config(golden["intonation"], golden["rhythm"]), golden["vocoid"], device=0)
    before = capi.postures_from_table(golden[ENTRY + "__postures"])
    feet, groups = capi.feet_from_table(golden[ENTRY + "__feet"]), capi.tone_groups_from_table(golden[ENTRY + "__groups"])
    after, status = prosody.rhythm_host(before, feet)
    events, rule_data, onsets, rule_status = rules.apply_host(4, after)
    assert status == 0 and rule_status == 0 and len(rule_data) <= MAX_RULES
    n, n_feet, n_groups, n_events = len(before), len(feet), len(groups), len(events)
    n_points = capi.prosody_point_count(n, feet, groups)
    draws = np.random.default_rng(4096).random((batch, n_feet, 2))
    events_capacity, points_capacity = batch * n_events, batch * n_points
    results = {"batch": batch, "postures": n, "feet": n_feet, "rules": len(rule_data), "events": n_events, "points": int(n_points), "reps": args.reps}

    def steps(count):
        return np.arange(batch + 1, dtype=np.int64) * count

    def device(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8) if a.dtype.names else np.ascontiguousarray(a)).cuda()

    d_before, d_after = device(np.tile(before, batch)), device(np.tile(after, batch))
    d_feet, d_groups, d_draws = device(np.tile(feet, batch)), device(np.tile(groups, batch)), device(draws.reshape(-1))
    d_po, d_fo, d_go = device(steps(n)), device(steps(n_feet)), device(steps(n_groups))
    d_voices = torch.zeros(batch, dtype=torch.int32, device="cuda")

    plan = g.VoicesPlan([g.config_from_dict(g.read_config_file(oracle.VOICE_MALE), 44100.0, 1, capi.PRECISION_F32)], 250.0, 0)
    config = capi.TrackConfig(control_period_ms=4, macro_intonation=1, micro_intonation=1, intonation_drift=0, smooth_intonation=1, initial_pitch=0.0,
                              mean_pitch=-12.0, drift_deviation=1.0, drift_sample_rate=250.0, drift_lowpass_cutoff=4.0)
    plan.set_voice_tracks([config])
    points0, status = prosody.points_host(4, after, feet, groups, draws[0], rule_data, onsets)
    merged0, _ = capi.intonation_apply_host(config, events, points0)
    max_frames = capi.tracks_frame_count(config, merged0) + 8
    stride = plan.voices_output_capacity(max_frames)
    results["frames"], results["samples_per_row"] = int(max_frames), int(stride)
    audio = [torch.zeros((batch, stride), dtype=torch.float32, device="cuda") for _ in range(2)]
    counts = [torch.zeros(batch, dtype=torch.int64, device="cuda") for _ in range(2)]
    peaks = [torch.zeros(batch, dtype=torch.float32, device="cuda") for _ in range(2)]
    statuses = [torch.zeros(batch, dtype=torch.int32, device="cuda") for _ in range(2)]
    placed = torch.zeros(batch, dtype=torch.int32, device="cuda")

    def new():
        plan.synthesize_prosody_device(rules, prosody, d_before, d_po, batch * n, d_feet, d_fo, batch * n_feet, d_groups, d_go, d_draws, d_voices, MAX_RULES,
                                       points_capacity, events_capacity, batch, max_frames, audio[0], stride, None, counts[0], peaks[0], None, placed, statuses[0],
                                       stream)

    if args.kernels:
        for _ in range(20):
            new()
        torch.cuda.synchronize()
        return

    # today's route: its device buffers, and the page-locked memory the rule data and the points cross in
    row = capi.RULE_DATA_DTYPE.itemsize
    d_gen = torch.empty(events_capacity * capi.EVENT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_gen_off = torch.empty(batch + 1, dtype=torch.int64, device="cuda")
    d_rows = torch.empty(batch * MAX_RULES * row, dtype=torch.uint8, device="cuda")
    d_counts, d_onsets = torch.empty(batch, dtype=torch.int32, device="cuda"), torch.empty(batch * n, dtype=torch.float64, device="cuda")
    d_rule_status = torch.empty(batch, dtype=torch.int32, device="cuda")
    h_rows, h_counts, h_onsets, h_rule_status = (torch.empty_like(t, device="cpu").pin_memory() for t in (d_rows, d_counts, d_onsets, d_rule_status))
    h_points = torch.empty(points_capacity * capi.POINT_DTYPE.itemsize, dtype=torch.uint8).pin_memory()
    h_point_off = torch.zeros(batch + 1, dtype=torch.int64).pin_memory()
    d_points, d_point_off = torch.empty_like(h_points, device="cuda"), torch.empty_like(h_point_off, device="cuda")
    h_after, h_feet, h_groups = np.tile(after, batch), np.tile(feet, batch), np.tile(groups, batch)
    point, posture, foot, group = capi.POINT_DTYPE.itemsize, capi.POSTURE_DTYPE.itemsize, capi.FOOT_DTYPE.itemsize, capi.TONE_GROUP_DTYPE.itemsize
    counts_view, status_view, offsets_view = h_counts.numpy(), h_rule_status.numpy(), h_point_off.numpy()
    n_out, status_out = ctypes.c_size_t(0), ctypes.c_int32(0)
    vp = ctypes.c_void_p
    fixed = [(vp(h_after.ctypes.data + b * n * posture), vp(h_feet.ctypes.data + b * n_feet * foot), vp(h_groups.ctypes.data + b * n_groups * group),
              vp(draws.ctypes.data + b * n_feet * 16), vp(h_rows.data_ptr() + b * MAX_RULES * row), vp(h_onsets.data_ptr() + b * n * 8)) for b in range(batch)]
    points_at = h_points.data_ptr()
    points_host = lib.gvtm_prosody_points_host

    def device_part():
        rules.generate_events_device(4, d_after, d_po, batch, d_gen, events_capacity, d_gen_off, d_rows, MAX_RULES, d_counts, d_onsets, d_rule_status, stream)
        h_rows.copy_(d_rows, non_blocking=True)
        h_counts.copy_(d_counts, non_blocking=True)
        h_onsets.copy_(d_onsets, non_blocking=True)
        h_rule_status.copy_(d_rule_status, non_blocking=True)
        torch.cuda.synchronize()

    def host_part():
        at = 0
        for b in range(batch):
            p, f, gr, d, r, o = fixed[b]
            rc = points_host(prosody._h, 4, p, n, f, n_feet, gr, n_groups, d, r, int(counts_view[b]), o, int(status_view[b]), vp(points_at + at * point),
                             points_capacity - at, ctypes.byref(n_out), ctypes.byref(status_out))
            assert rc == 0 and status_out.value == 0
            at += n_out.value
            offsets_view[b + 1] = at

    def empty_loop():
        for b in range(batch):
            lib.gvtm_prosody_point_count(0, None, 0, None, 0)

    def today():
        device_part()
        host_part()
        d_points.copy_(h_points, non_blocking=True)
        d_point_off.copy_(h_point_off, non_blocking=True)
        plan.synthesize_intonation_device(d_gen, d_gen_off, batch, None, d_points, d_point_off, d_voices, events_capacity + points_capacity, batch, max_frames,
                                          audio[1], stride, None, counts[1], peaks[1], None, statuses[1], stream)

    new()
    today()
    torch.cuda.synchronize()
    assert (placed == 0).all() and (statuses[0] == 0).all() and torch.equal(statuses[0], statuses[1])
    assert torch.equal(counts[0], counts[1]) and torch.equal(peaks[0], peaks[1]) and torch.equal(audio[0], audio[1]), "the two routes' samples differ"
    assert not torch.equal(audio[0][0], audio[0][1]), "every utterance has draws of its own"
    results["samples_compared"] = int(counts[0].sum().item())

    fns = {"new": new, "today": today, "today_device_part": device_part, "today_host_loop": host_part, "empty_ctypes_loop": empty_loop}
    for fn in fns.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(args.reps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    for k, v in times.items():
        results[k + "_ms"], results[k + "_span"] = float(np.median(v)), [min(v), max(v)]
    print(json.dumps(results))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
