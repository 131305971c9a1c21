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
import oracle  # noqa: E402

VOICES = ["male", "female", "large_child", "small_child", "baby"]


def track_config(voice):
    """0_male/vtm_control_model.txt with mean pitch = pitch offset (-4) + the variant's reference_glottal_pitch"""
    tc = g.TrackConfig()
    tc.control_period_ms, tc.macro_intonation, tc.micro_intonation, tc.intonation_drift, tc.smooth_intonation = 4, 1, 1, 1, 1
    tc.initial_pitch, tc.drift_deviation, tc.drift_sample_rate, tc.drift_lowpass_cutoff = -20.0, 4.0, 250.0, 4.0
    tc.mean_pitch = -4.0 + float(g.read_config_file(os.path.join(oracle.GOLDEN_DIR, "voice_%s.txt" % voice))["reference_glottal_pitch"])
    return tc


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


def on_device(evs):
    offsets = np.zeros(len(evs) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(e) for e in evs])
    return torch.from_numpy(np.concatenate(evs).view(np.uint8)).cuda(), torch.from_numpy(offsets).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--skip-synthesis", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    batch = args.batch
    stream = torch.cuda.current_stream().cuda_stream
    tcs = [track_config(v) for v in VOICES]
    cfgs = [g.config_from_dict(g.read_config_file(os.path.join(oracle.GOLDEN_DIR, "voice_%s.txt" % n)), 44100.0, 1, capi.PRECISION_F32) for n in VOICES]
    plan = g.VoicesPlan(cfgs, 250.0, 0)
    plan.set_voice_tracks(tcs)
    results = {"batch": batch, "events_per_list": 80, "reps": args.reps, "voices": VOICES}

    # --- track generation alone: bench_tracks.py's lists
    tables = [event_lists.random_event_table(s, n_events=80, control_period=4, max_gap_periods=12) for s in range(64)]
    pool = [capi.events_from_table(t) for t in tables]
    max_frames = max(capi.tracks_frame_count(tcs[0], e) for e in pool)
    d_events, d_offsets = on_device([pool[b % 64] for b in range(batch)])
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

    # --- end to end, float: lists the models can sing (test_gpu_tracks._singable_event_table's polynomials)
    if not args.skip_synthesis:
        for t in tables:
            t[:, 2] = 0.0
            t[:, 3] = 0.0
            t[:, 4] *= 0.1
            t[:, 5] *= 0.5
        pool = [capi.events_from_table(t) for t in tables]
        lists = [pool[b % 64] for b in range(batch)]
        d_events, d_offsets = on_device(lists)
        stride = plan.voices_output_capacity(max_frames)
        audio = torch.zeros((batch, stride), dtype=torch.float32, device="cuda")
        counts = torch.zeros(batch, dtype=torch.int64, device="cuda")
        singles = [g.Plan(c, 250.0, 0) for c in cfgs]
        per_voice = []
        for v in range(len(VOICES)):
            sel = np.nonzero(ids == v)[0]
            ev, off = on_device([lists[b] for b in sel])
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
