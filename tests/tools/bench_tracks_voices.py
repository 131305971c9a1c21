"""GPU-box: event lists of a batch that mixes voices (gvtm_generate_tracks_voices_device,
gvtm_synthesize_events_voices_device).

bench_tracks.py's lists (4096 x 80 events, ~500 frames each), the five GamaTTS variants interleaved, everything resident:
  tracks      the single-configuration kernel (gvtm_generate_tracks_device), the voice variant with the five voices
              interleaved (the two rows of a wavefront always of different voices) and with one voice id for the whole batch
              (the per-lane constants without the divergence by voice)
  end to end  one gvtm_synthesize_events_voices_device call against the same lists grouped by voice through five
              gvtm_synthesize_events_device calls, one single-voice plan each, back to back (float)
The variants of a comparison alternate inside every repeat; medians, wall time between HIP events.
usage: python tests/tools/bench_tracks_voices.py [--reps N] [--skip-synthesis] [--out FILE.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import gama_tts_amd as g  # noqa: E402
from gama_tts_amd import capi  # noqa: E402
import event_lists  # noqa: E402
from device_io import events_on_device  # noqa: E402
from track_cases import make_singable  # noqa: E402
from voice_cases import configs, track_configs  # noqa: E402
from voice_files import VOICES  # noqa: E402


def timed_alternating(fns, reps, inner):
    """{name: median ms per call}: every repeat times each variant once (`inner` calls between two events)."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            torch.cuda.synchronize()
            times[k].append(a.elapsed_time(b) / inner)
    return {k: float(np.median(v)) for k, v in times.items()}, {k: [min(v), max(v)] for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--skip-synthesis", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    batch = args.batch
    stream = torch.cuda.current_stream().cuda_stream
    tcs = track_configs()
    cfgs = configs(precision=capi.PRECISION_F32)
    plan = g.VoicesPlan(cfgs, 250.0, 0)
    plan.set_voice_tracks(tcs)
    results = {"batch": batch, "events_per_list": 80, "reps": args.reps, "voices": VOICES}

    # --- track generation alone: bench_tracks.py's lists
    tables = [event_lists.random_event_table(s, n_events=80, control_period=4, max_gap_periods=12) for s in range(64)]
    max_frames = max(capi.tracks_frame_count(tcs[0], capi.events_from_table(t)) for t in tables)
    d_events, d_offsets = events_on_device([tables[b % 64] for b in range(batch)])
    ids = (np.arange(batch) % len(VOICES)).astype(np.int32)
    d_ids = torch.from_numpy(ids).cuda()
    d_one = torch.zeros(batch, dtype=torch.int32, device="cuda")
    d_params = torch.zeros((batch, max_frames, 16), dtype=torch.float32, device="cuda")
    d_counts = torch.zeros(batch, dtype=torch.int32, device="cuda")
    med, spread = timed_alternating({
        "single_configuration_ms": lambda: capi.generate_tracks_device(tcs[0], d_events, d_offsets, batch, max_frames, d_params, d_counts, None, stream),
        "voices_interleaved_ms": lambda: plan.generate_tracks_voices_device(d_events, d_offsets, d_ids, batch, max_frames, d_params, d_counts, None, stream),
        "voices_one_voice_ms": lambda: plan.generate_tracks_voices_device(d_events, d_offsets, d_one, batch, max_frames, d_params, d_counts, None, stream),
    }, args.reps, 20)
    results["tracks"] = dict(med, min_max=spread, frames_total=int(d_counts.sum().item()),
                             voices_over_single=med["voices_interleaved_ms"] / med["single_configuration_ms"])
    print(json.dumps({"tracks": results["tracks"]}), flush=True)
    del d_params

    # --- end to end, float: lists the models can sing (track_cases.singable_event_table's polynomials)
    if not args.skip_synthesis:
        singable = [make_singable(t) for t in tables]
        lists = [singable[b % 64] for b in range(batch)]
        d_events, d_offsets = events_on_device(lists)
        stride = plan.voices_output_capacity(max_frames)
        audio = torch.zeros((batch, stride), dtype=torch.float32, device="cuda")
        counts = torch.zeros(batch, dtype=torch.int64, device="cuda")
        singles = [g.Plan(c, 250.0, 0) for c in cfgs]
        per_voice = []
        for v in range(len(VOICES)):
            sel = np.nonzero(ids == v)[0]
            ev, off = events_on_device([lists[b] for b in sel])
            per_voice.append((ev, off, sel.size, torch.zeros((sel.size, stride), dtype=torch.float32, device="cuda"),
                              torch.zeros(sel.size, dtype=torch.int64, device="cuda")))

        def mixed():
            plan.synthesize_events_voices_device(d_events, d_offsets, d_ids, batch, max_frames, audio, stride, None, counts, None, None, stream)

        def sequential():
            for v, (ev, off, n, a, c) in enumerate(per_voice):
                singles[v].synthesize_events_device(tcs[v], ev, off, n, max_frames, a, stride, None, c, None, None, stream)

        med, spread = timed_alternating({"events_voices_ms": mixed, "five_single_voice_launches_ms": sequential}, args.reps, 1)
        # the two ways give the same samples
        mixed()
        sequential()
        torch.cuda.synchronize()
        same = all(torch.equal(audio[torch.from_numpy(np.nonzero(ids == v)[0]).cuda()].view(torch.int32), per_voice[v][3].view(torch.int32))
                   for v in range(len(VOICES)))
        results["end_to_end_f32"] = dict(med, min_max=spread, samples_total=int(counts.sum().item()), same_samples=bool(same),
                                         mixed_over_sequential=med["events_voices_ms"] / med["five_single_voice_launches_ms"])
        print(json.dumps({"end_to_end_f32": results["end_to_end_f32"]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
