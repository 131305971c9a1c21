"""GPU-box: several voices of the float class of reference model 5 in one launch against one launch per voice
(gvtm_plan_create_model5_float_voices): what bench_voices5.py measures for the double class, in float.

The five variants of 5_male (242 to 564 internal steps per 250 Hz frame) interleaved over a batch of 500-frame utterances
(2 s, 48 kHz), N utterances per voice, timed on the device, everything resident:
  mixed          one gvtm_synthesize_voices_device call (grouping kernel + one synthesis launch), voices in plan order
                 male .. baby
  mixed_longest  the same with the plan's voices in the opposite order (baby .. male): the longest utterances first
  sequential     the same utterances as five gvtm_synthesize_batch_device calls, one gvtm_plan_create_model5_float plan
                 each, back to back: the code a caller had before plans of several float voices
  single         one gvtm_synthesize_batch_device call of a male-only batch of the same size
for N = 16 / 52 / 256 / 1024.  Every variant of a size is warmed up first; the repeats then alternate the variants (one of
each per round), so that what else the machine does falls on all of them alike.  Per variant: the median, the fastest and
the slowest repeat and spread = (slowest - fastest) / median, wall time between HIP events.
usage: python tests/tools/bench_voices5_float.py [--reps N] [--frames F] [--per-voice 16,52,...] [--out FILE.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import gama_tts_amd as g  # noqa: E402
import model5_cases as cases  # noqa: E402
import tracks  # noqa: E402
from voice_files import VOICES  # noqa: E402
from voices5_float_cases import configs5f, single_float_plan  # noqa: E402

VARIANTS = ["mixed", "mixed_longest_first", "sequential", "single_voice"]


def timed_alternating(fns, reps):
    """Every function once to warm up, then `reps` rounds of one timed call of each -> {name: [ms per repeat]}."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b))
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", type=int, default=500)
    ap.add_argument("--per-voice", default="16,52,256,1024")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 5:
        sys.exit("at least five repeats per variant")
    frames = args.frames
    stream = torch.cuda.current_stream().cuda_stream
    cfgs = configs5f(cases.RATE)
    mixed_plan = g.VoicesPlan(cfgs, 250.0, 0, float_model5=True)
    reversed_plan = g.VoicesPlan(cfgs[::-1], 250.0, 0, float_model5=True)
    singles = [single_float_plan(c) for c in cfgs]
    base = torch.from_numpy(tracks.random_tracks(64, frames, seed0=1000, consonant_heavy=True)).cuda()
    stride = mixed_plan.voices_output_capacity(frames)
    steps = [mixed_plan.voice_info(v).control_steps for v in range(len(VOICES))]
    results = {"class": "VocalTractModel5<float,1>", "frames": frames, "reps": args.reps, "output_rate": cases.RATE, "voices": VOICES,
               "steps_per_frame": steps, "compute_units": torch.cuda.get_device_properties(0).multi_processor_count, "rows": []}
    for per_voice in [int(x) for x in args.per_voice.split(",")]:
        batch = per_voice * len(VOICES)
        params = base[torch.arange(batch, device="cuda") % 64].contiguous()
        ids = torch.from_numpy((np.arange(batch) % len(VOICES)).astype(np.int32)).cuda()  # interleaved
        ids_rev = (len(VOICES) - 1 - ids).contiguous()
        audio = torch.empty((batch, stride), dtype=torch.float32, device="cuda")
        counts = torch.zeros(batch, dtype=torch.int64, device="cuda")
        per = []
        for v in range(len(VOICES)):
            sel = torch.nonzero(ids == v).flatten()
            per.append((params[sel].contiguous(), torch.empty((sel.numel(), stride), dtype=torch.float32, device="cuda"),
                        torch.zeros(sel.numel(), dtype=torch.int64, device="cuda")))

        def mixed():
            mixed_plan.synthesize_voices_device(params, ids, batch, frames, audio, stride, None, counts, None, stream)

        def mixed_longest():
            reversed_plan.synthesize_voices_device(params, ids_rev, batch, frames, audio, stride, None, counts, None, stream)

        def sequential():
            for v, (p, a, c) in enumerate(per):
                singles[v].synthesize_device(p, p.shape[0], frames, a, stride, None, c, None, stream)

        def single():
            singles[0].synthesize_device(params, batch, frames, audio, stride, None, counts, None, stream)

        times = timed_alternating(dict(zip(VARIANTS, [mixed, mixed_longest, sequential, single])), args.reps)
        # the internal steps of the mixed batch, for a rate that compares with the single-voice benchmarks'
        row = {"per_voice": per_voice, "batch": batch, "internal_steps": per_voice * frames * sum(steps)}
        for name in VARIANTS:
            t = np.array(times[name])
            row[name + "_ms"] = float(np.median(t))
            row[name + "_min_ms"], row[name + "_max_ms"] = float(t.min()), float(t.max())
            row[name + "_spread"] = float((t.max() - t.min()) / np.median(t))
        row["mixed_over_sequential"] = row["mixed_ms"] / row["sequential_ms"]
        row["sequential_over_mixed"] = row["sequential_ms"] / row["mixed_ms"]
        row["mixed_gsteps_per_s"] = row["internal_steps"] / row["mixed_ms"] / 1e6
        results["rows"].append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
