"""GPU-box: the float class of reference model 5 (gvtm_plan_create_model5_float) against the fp64 plan, kernel time only.

5_male at 48 kHz, 500-frame utterances (2 s), batches of 256 / 512 / 4096, everything resident, timed by the plan's own
HIP events (gvtm_plan_take_kernel_ms), median of the repeats after a warm-up, all in one process:
  f64 (x3)     the fp64 plan, three separate legs, so that the run-to-run spread is on record
  f32          the float plan as the product launches it (synth_launch_shape picks the shape by batch size)
  f32_chunk60  the float plan forced to its chunk-60 shape (diagnostics library, rows 1): one workgroup per compute unit
  f32_chunk56  the float plan forced to its chunk-56 shape (rows 2): 80 KB of LDS, two workgroups per compute unit
usage: python tests/tools/bench_model5_float.py [--reps N] [--frames F] [--batches 256,512,4096] [--out FILE.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import gama_tts_amd as g  # noqa: E402
import oracle  # noqa: E402
import tracks  # noqa: E402
from gama_tts_amd import capi  # noqa: E402

RATE = 48000.0


def kernel_ms(plan, fn, reps):
    """Median kernel time of `reps` launches of fn() after one warm-up launch."""
    fn()
    torch.cuda.synchronize()
    plan.take_kernel_ms()
    times = []
    for _ in range(reps):
        fn()
        torch.cuda.synchronize()
        ms, n = plan.take_kernel_ms()
        assert n == 1, n
        times.append(ms)
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=500)
    ap.add_argument("--batches", default="256,512,4096")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    frames = args.frames
    stream = torch.cuda.current_stream().cuda_stream
    d = g.read_config_file(oracle.VOICE5_MALE)
    cfg64 = g.config5_from_dict(d, RATE)
    cfg32 = g.config5_from_dict(d, RATE, capi.PRECISION_F32)
    legs = [("f64_a", g.Plan(cfg64, 250.0, 0)), ("f64_b", g.Plan(cfg64, 250.0, 0)), ("f64_c", g.Plan(cfg64, 250.0, 0)),
            ("f32", g.Plan(cfg32, 250.0, 0, float_model5=True)),
            ("f32_chunk60", g.Plan(cfg32, 250.0, 0, diagnostics=True, rows=1, float_model5=True)),
            ("f32_chunk56", g.Plan(cfg32, 250.0, 0, diagnostics=True, rows=2, float_model5=True))]
    for _, plan in legs:
        plan.set_timing(True)
    base = torch.from_numpy(tracks.random_tracks(64, frames, seed0=1000, consonant_heavy=True)).cuda()
    results = {"frames": frames, "reps": args.reps, "output_rate": RATE, "voice": "5_male",
               "compute_units": torch.cuda.get_device_properties(0).multi_processor_count, "rows": []}
    for batch in [int(x) for x in args.batches.split(",")]:
        params = base[torch.arange(batch, device="cuda") % 64].contiguous()
        row = {"batch": batch}
        for name, plan in legs:
            stride = plan.output_capacity(frames)
            audio = torch.empty((batch, stride), dtype=torch.float32, device="cuda")
            counts = torch.zeros(batch, dtype=torch.int64, device="cuda")
            ms = kernel_ms(plan, lambda: plan.synthesize_device(params, batch, frames, audio, stride, None, counts, None, stream), args.reps)
            row[name + "_ms"] = ms
            row[name + "_gsamples_per_s"] = float(counts.sum().item()) / ms / 1e6
            del audio
        f64 = [row["f64_a_ms"], row["f64_b_ms"], row["f64_c_ms"]]
        row["f64_spread_ms"] = max(f64) - min(f64)
        row["f64_median_ms"] = float(np.median(f64))
        row["f32_speedup"] = row["f64_median_ms"] / row["f32_ms"]
        results["rows"].append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
