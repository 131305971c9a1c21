"""GPU-box: several reference model 5 voices in one launch against one launch per voice (gvtm_plan_create_model5_voices,
DESIGN.md 10).

The five variants of 5_male (tests/golden/voice5_*.txt: 242 to 564 internal steps per 250 Hz frame) interleaved over a
batch of 500-frame utterances (2 s, 48 kHz), N utterances per voice, timed on the device, everything resident:
  mixed          one gvtm_synthesize_voices_device call (grouping kernel + one synthesis launch), voices in plan order
                 male .. baby, so the workgroups of the voice with the fewest steps per frame are dispatched first
  mixed_longest  the same with the plan's voices in the opposite order (baby .. male): the longest utterances first
  sequential     the same utterances as five gvtm_synthesize_batch_device calls, one single-voice plan each, back to back
  single         one gvtm_synthesize_batch_device call of a male-only batch of the same size
for N = 16 / 52 / 256 / 1024.  Median of the repeats, wall time between HIP events.
usage: python tests/tools/bench_voices5.py [--reps N] [--frames F] [--out FILE.json]"""
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
from voice_cases import configs5  # noqa: E402
from voice_files import VOICES  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=500)
    ap.add_argument("--per-voice", default="16,52,256,1024")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    frames = args.frames
    stream = torch.cuda.current_stream().cuda_stream
    cfgs = configs5(cases.RATE)
    mixed_plan = g.VoicesPlan(cfgs, 250.0, 0)
    reversed_plan = g.VoicesPlan(cfgs[::-1], 250.0, 0)
    singles = [g.Plan(c, 250.0, 0) for c in cfgs]
    base = torch.from_numpy(tracks.random_tracks(64, frames, seed0=1000, consonant_heavy=True)).cuda()
    stride = mixed_plan.voices_output_capacity(frames)
    results = {"frames": frames, "reps": args.reps, "output_rate": cases.RATE, "voices": VOICES,
               "steps_per_frame": [mixed_plan.voice_info(v).control_steps for v in range(len(VOICES))],
               "compute_units": torch.cuda.get_device_properties(0).multi_processor_count, "rows": []}
    for per_voice in [int(x) for x in args.per_voice.split(",")]:
        batch = per_voice * len(VOICES)
        params = base[torch.arange(batch, device="cuda") % 64].contiguous()
        ids = torch.from_numpy((np.arange(batch) % len(VOICES)).astype(np.int32)).cuda()  # interleaved
        ids_rev = (len(VOICES) - 1 - ids).contiguous()
        audio = torch.empty((batch, stride), dtype=torch.float32, device="cuda")
        counts = torch.zeros(batch, dtype=torch.int64, device="cuda")

        def mixed():
            mixed_plan.synthesize_voices_device(params, ids, batch, frames, audio, stride, None, counts, None, stream)

        def mixed_longest():
            reversed_plan.synthesize_voices_device(params, ids_rev, batch, frames, audio, stride, None, counts, None, stream)

        per = []
        for v in range(len(VOICES)):
            sel = torch.nonzero(ids == v).flatten()
            per.append((params[sel].contiguous(), torch.empty((sel.numel(), stride), dtype=torch.float32, device="cuda"),
                        torch.zeros(sel.numel(), dtype=torch.int64, device="cuda")))

        def sequential():
            for v, (p, a, c) in enumerate(per):
                singles[v].synthesize_device(p, p.shape[0], frames, a, stride, None, c, None, stream)

        def single():
            singles[0].synthesize_device(params, batch, frames, audio, stride, None, counts, None, stream)

        row = {"per_voice": per_voice, "batch": batch, "mixed_ms": timed(mixed, args.reps),
               "mixed_longest_first_ms": timed(mixed_longest, args.reps), "sequential_ms": timed(sequential, args.reps),
               "single_voice_ms": timed(single, args.reps)}
        row["sequential_over_mixed"] = row["sequential_ms"] / row["mixed_ms"]
        results["rows"].append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
