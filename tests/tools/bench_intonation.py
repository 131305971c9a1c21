"""GPU-box: intonation contours applied to event lists on the device (gvtm_apply_intonation_device,
gvtm_synthesize_intonation_device).

4096 utterances x 80 base events x 12 points, everything resident, once with a base list per utterance and once with one
list shared by all of them:
  apply       the three apply kernels together (one gvtm_apply_intonation_device call), with the achieved GB/s on the
              algorithmic bytes, 296 x (E read + M written) + 24 x P per utterance
  tracks      the tracks kernel (gvtm_generate_tracks_voices_device) on the same merged lists, in the same process
  end to end  one gvtm_synthesize_intonation_device call (float) against the existing path fed lists merged on the host:
              the merged events copied from page-locked memory, then gvtm_synthesize_events_voices_device.  The host's
              merging itself (gvtm_intonation_apply_host per utterance) is timed apart and not part of either figure.
The variants of a comparison alternate inside every repeat; medians, wall time between HIP events.
usage: python tests/tools/bench_intonation.py [--reps N] [--batch B] [--skip-synthesis] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import gama_tts_amd as g  # noqa: E402
from gama_tts_amd import capi  # noqa: E402
import event_lists  # noqa: E402
from bench_tracks_voices import timed_alternating  # noqa: E402
from track_cases import make_singable  # noqa: E402
from voice_cases import configs, track_configs  # noqa: E402

EVENTS, POINTS = 80, 12
EVENT_BYTES, POINT_BYTES = capi.EVENT_DTYPE.itemsize, capi.POINT_DTYPE.itemsize


def contour(table, seed):
    """12 points on distinct control periods up to the last event, on a gentle curve with its own slopes (the cubic through
    them stays inside the range the models can sing)."""
    rng = np.random.default_rng(seed)
    slots = np.sort(rng.choice(np.arange(1, int(table[-1, 0]) // 4), POINTS, replace=False))
    t = slots * 4.0 + rng.uniform(0.0, 3.9, POINTS)
    phase, rate = rng.uniform(0, 6.28), rng.uniform(1 / 400.0, 1 / 150.0)
    return np.stack([t, 3.0 * np.sin(phase + t * rate), 3.0 * rate * np.cos(phase + t * rate)], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--skip-synthesis", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    batch = args.batch
    stream = torch.cuda.current_stream().cuda_stream
    tc = track_configs(names=["male"])
    plan = g.VoicesPlan(configs(precision=capi.PRECISION_F32, names=["male"]), 250.0, 0)
    plan.set_voice_tracks(tc)
    results = {"batch": batch, "events_per_list": EVENTS, "points": POINTS, "reps": args.reps}

    tables = [make_singable(event_lists.random_event_table(s, n_events=EVENTS, control_period=4, max_gap_periods=12)) for s in range(64)]
    events = [capi.events_from_table(t) for t in tables]
    points = [contour(tables[b % 64], b) for b in range(batch)]
    t0 = time.perf_counter()
    merged = [capi.intonation_apply_host(tc[0], events[b % 64], capi.points_from_table(points[b]))[0] for b in range(batch)]
    results["host_merge_s_through_the_binding"] = time.perf_counter() - t0
    merged_total = sum(len(m) for m in merged)
    max_frames = max(capi.tracks_frame_count(tc[0], m) for m in merged)
    capacity = batch * (EVENTS + POINTS)
    algorithmic = EVENT_BYTES * (batch * EVENTS + merged_total) + POINT_BYTES * batch * POINTS
    results.update(merged_events=merged_total, max_frames=max_frames, algorithmic_bytes=algorithmic,
                   upload_bytes_points=POINT_BYTES * batch * POINTS, upload_bytes_merged_events=EVENT_BYTES * merged_total)

    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    d_points = dev(np.concatenate(points))
    d_points_shared = dev(np.concatenate([contour(tables[0], b) for b in range(batch)]))  # (every contour inside list 0's duration)
    d_point_offsets = dev(np.arange(batch + 1, dtype=np.int64) * POINTS)
    d_voices = torch.zeros(batch, dtype=torch.int32, device="cuda")
    layouts = {
        "own": (dev(np.concatenate([events[b % 64] for b in range(batch)]).view(np.uint8)), dev(np.arange(batch + 1, dtype=np.int64) * EVENTS), batch, None),
        "shared": (dev(events[0].view(np.uint8)), dev(np.array([0, EVENTS], dtype=np.int64)), 1, torch.zeros(batch, dtype=torch.int32, device="cuda")),
    }
    d_out = torch.zeros(capacity * EVENT_BYTES, dtype=torch.uint8, device="cuda")
    d_offsets = torch.zeros(batch + 1, dtype=torch.int64, device="cuda")
    d_status = torch.zeros(batch, dtype=torch.int32, device="cuda")
    d_params = torch.zeros((batch, max_frames, 16), dtype=torch.float32, device="cuda")
    d_counts = torch.zeros(batch, dtype=torch.int32, device="cuda")

    def apply(layout):
        ev, off, n_lists, ids = layouts[layout]
        plan.apply_intonation_device(ev, off, n_lists, ids, d_points if ids is None else d_points_shared, d_point_offsets, d_voices, batch, d_out, capacity,
                                     d_offsets, d_status, stream)

    def tracks():
        plan.generate_tracks_voices_device(d_out, d_offsets, d_voices, batch, max_frames, d_params, d_counts, None, stream)

    # the device's lists are the host's (own lists), before anything is timed
    apply("own")
    torch.cuda.synchronize()
    assert int(d_status.abs().sum().item()) == 0 and int(d_offsets[-1].item()) == merged_total
    same = d_out[: merged_total * EVENT_BYTES].cpu().numpy().tobytes() == np.concatenate(merged).tobytes()
    results["device_lists_equal_host_lists"] = bool(same)
    med, spread = timed_alternating({"apply_own_ms": lambda: apply("own"), "apply_shared_ms": lambda: apply("shared"), "tracks_ms": tracks}, args.reps, 50)
    apply("shared")
    torch.cuda.synchronize()
    assert int(d_status.abs().sum().item()) == 0
    shared_total = int(d_offsets[-1].item())
    shared_bytes = EVENT_BYTES * (batch * EVENTS + shared_total) + POINT_BYTES * batch * POINTS
    results["kernels"] = dict(med, min_max=spread, apply_own_gb_s=algorithmic / med["apply_own_ms"] / 1e6,
                              apply_own_over_tracks=med["apply_own_ms"] / med["tracks_ms"],
                              apply_shared_over_tracks=med["apply_shared_ms"] / med["tracks_ms"], shared_merged_events=shared_total,
                              apply_shared_gb_s=shared_bytes / med["apply_shared_ms"] / 1e6)
    print(json.dumps({"kernels": results["kernels"]}), flush=True)
    del d_params

    if not args.skip_synthesis:
        stride = plan.voices_output_capacity(max_frames)
        audio = [torch.zeros((batch, stride), dtype=torch.float32, device="cuda") for _ in range(2)]
        counts = [torch.zeros(batch, dtype=torch.int64, device="cuda") for _ in range(2)]
        pinned = torch.from_numpy(np.concatenate(merged).view(np.uint8)).pin_memory()
        host_offsets = np.zeros(batch + 1, dtype=np.int64)
        host_offsets[1:] = np.cumsum([len(m) for m in merged])
        pinned_offsets = torch.from_numpy(host_offsets).pin_memory()
        d_merged = torch.zeros(merged_total * EVENT_BYTES, dtype=torch.uint8, device="cuda")
        d_merged_offsets = torch.zeros(batch + 1, dtype=torch.int64, device="cuda")
        pinned_points = torch.from_numpy(np.concatenate(points)).pin_memory()
        ev, off, n_lists, ids = layouts["own"]

        def one_call():  # the points are what differs between utterances: they cross the bus, the base lists are resident
            d_points.copy_(pinned_points, non_blocking=True)
            plan.synthesize_intonation_device(ev, off, n_lists, ids, d_points, d_point_offsets, d_voices, capacity, batch, max_frames, audio[0], stride,
                                              None, counts[0], None, None, None, stream)

        def host_merged():
            d_merged.copy_(pinned, non_blocking=True)
            d_merged_offsets.copy_(pinned_offsets, non_blocking=True)
            plan.synthesize_events_voices_device(d_merged, d_merged_offsets, d_voices, batch, max_frames, audio[1], stride, None, counts[1], None, None, stream)

        med, spread = timed_alternating({"one_call_ms": one_call, "host_merged_lists_ms": host_merged}, args.reps, 1)
        one_call()
        host_merged()
        torch.cuda.synchronize()
        results["end_to_end_f32"] = dict(med, min_max=spread, samples_total=int(counts[0].sum().item()),
                                         same_samples=bool(torch.equal(audio[0].view(torch.int32), audio[1].view(torch.int32))),
                                         one_call_over_host_merged=med["one_call_ms"] / med["host_merged_lists_ms"])
        print(json.dumps({"end_to_end_f32": results["end_to_end_f32"]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
