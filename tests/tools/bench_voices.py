"""GPU-box: several voices in one launch against one launch per voice (gvtm_synthesize_voices_device).

The five GamaTTS variants (tests/golden/voice_*.txt) interleaved over a batch of 500-frame utterances (2 s), timed three ways
on the device, everything resident:
  mixed       one gvtm_synthesize_voices_device call (grouping kernel + one synthesis launch)
  sequential  the same utterances as five gvtm_synthesize_batch_device calls, one single-voice plan each, back to back
  single      one gvtm_synthesize_batch_device call of a male-only batch of the same size
at batch 4096 and at 1280 (about 256 utterances per voice).  Median of the repeats, wall time between HIP events.
usage: python tests/tools/bench_voices.py [--reps N] [--precision f32|mixed|f64] [--out FILE.json]"""
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
import tracks  # noqa: E402
from voice_cases import configs  # noqa: E402
from voice_files import VOICES  # noqa: E402

PRECISIONS = {"f32": capi.PRECISION_F32, "mixed": capi.PRECISION_MIXED, "f64": capi.PRECISION_F64}


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
    ap.add_argument("--precision", default="f32", choices=sorted(PRECISIONS))
    ap.add_argument("--frames", type=int, default=500)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    prec = PRECISIONS[args.precision]
    frames = args.frames
    stream = torch.cuda.current_stream().cuda_stream
    cfgs = configs(precision=prec)
    mixed_plan = g.VoicesPlan(cfgs, 250.0, 0)
    singles = [g.Plan(c, 250.0, 0) for c in cfgs]
    base = torch.from_numpy(tracks.random_tracks(64, frames, seed0=1000)).cuda()
    stride = mixed_plan.voices_output_capacity(frames)
    results = {"precision": args.precision, "frames": frames, "reps": args.reps, "voices": VOICES, "rows": []}
    for batch in (4096, 1280):
        params = base[torch.arange(batch, device="cuda") % 64].contiguous()
        ids = torch.from_numpy((np.arange(batch) % len(VOICES)).astype(np.int32)).cuda()  # interleaved
        audio = torch.empty((batch, stride), dtype=torch.float32, device="cuda")
        counts = torch.zeros(batch, dtype=torch.int64, device="cuda")

        def mixed():
            mixed_plan.synthesize_voices_device(params, ids, batch, frames, audio, stride, None, counts, None, stream)

        per_voice = []
        for v in range(len(VOICES)):
            sel = torch.nonzero(ids == v).flatten()
            per_voice.append((params[sel].contiguous(), torch.empty((sel.numel(), stride), dtype=torch.float32, device="cuda"),
                              torch.zeros(sel.numel(), dtype=torch.int64, device="cuda")))

        def sequential():
            for v, (p, a, c) in enumerate(per_voice):
                singles[v].synthesize_device(p, p.shape[0], frames, a, stride, None, c, None, stream)

        def single():
            singles[0].synthesize_device(params, batch, frames, audio, stride, None, counts, None, stream)

        row = {"batch": batch, "mixed_ms": timed(mixed, args.reps), "sequential_ms": timed(sequential, args.reps),
               "single_voice_ms": timed(single, args.reps)}
        row["mixed_over_sequential"] = row["mixed_ms"] / row["sequential_ms"]
        results["rows"].append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
