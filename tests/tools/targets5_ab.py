"""GPU-box: model 5 from parameter targets (gvtm_synthesize_targets_model5_device) beside the only route the
parent commit has for such data, on the same utterances, in both classes.

5_male at 48 kHz (internal rate 60 411 Hz, filter of 3021 samples); utterances of 60 000 internal steps, about 20 points per
parameter, a pool of 16 distinct utterances tiled over the batch.
  A     the new entry: target lists in (shared through list ids), the moving averages in the kernel
  B     gvtm_synthesize_batch_device on a plan whose control rate is the internal rate (one step per frame), fed the frames
        gvtm_targets_apply_host makes of the same lists: 64 bytes per step and utterance, expanded before the clock starts.
        Its samples are the batch protocol's, NOT the interactive model's: the comparison is of time and bytes read only
  A60 / A52   (float class) the new entry with either shape forced, a diagnostics plan's rows 1 / rows 2: chunk 60, one
        workgroup per compute unit, against chunk 52, two
The routes alternate inside every repeat; medians and the spread of the repeats, time between HIP events after warm-up.
Before anything is timed, A's rows are compared with each other across the tiling (copies of one pool member must be equal).
usage: python tests/tools/targets5_ab.py [--reps N] [--batches 256,4096] [--steps S] [--out FILE.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
from gama_tts_amd import capi  # noqa: E402
import targets_cases as cases  # noqa: E402
from bench_tracks_voices import timed_alternating  # noqa: E402
from voice_cases import model5_plan  # noqa: E402

POOL = 16


def measure(float_class, batch, steps, reps):
    stream = torch.cuda.current_stream().cuda_stream
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    plan = model5_plan(float_class=float_class)
    rate = plan.info.internal_rate_hz
    frames_plan = model5_plan(float_class=float_class, crate=rate)
    assert frames_plan.info.control_steps == 1 and frames_plan.info.internal_rate_hz == rate
    stride = plan.targets_output_capacity(steps)
    assert stride == frames_plan.output_capacity(steps)

    pool = [cases.spoken_lists(steps, seed, stride=steps // 20 + 7) for seed in range(POOL)]
    points = sum(len(l[0]) for u in pool for l in u)
    offsets, p_steps, p_values = capi.pack_targets([l for u in pool for l in u])
    ids = (np.arange(batch)[:, None] % POOL * 16 + np.arange(16)[None, :]).astype(np.int32)
    d_offsets, d_steps, d_values, d_ids = dev(offsets), dev(p_steps), dev(p_values), dev(ids)
    # B's frames: the pool's through the host rule, tiled on the device
    pool_frames = np.stack([capi.targets_apply_host(plan, u, steps)[0] for u in pool])
    d_params = dev(pool_frames).repeat((batch + POOL - 1) // POOL, 1, 1)[:batch].contiguous()
    names = ["A", "B"] + (["A60", "A52"] if float_class else [])
    audio = {k: torch.zeros((batch, stride), dtype=torch.float32, device="cuda") for k in names}
    counts = {k: torch.zeros(batch, dtype=torch.int64, device="cuda") for k in names}
    d_status = torch.zeros(batch, dtype=torch.int32, device="cuda")

    def entry(p, k):
        return lambda: p.synthesize_targets_model5_device(d_offsets, POOL * 16, d_ids, d_steps, d_values, None, batch, steps, audio[k], stride,
                                                          counts[k], None, d_status, stream)

    fns = {"A_ms": entry(plan, "A"),
           "B_ms": lambda: frames_plan.synthesize_device(d_params, batch, steps, audio["B"], stride, None, counts["B"], None, stream)}
    if float_class:
        fns["A60_ms"] = entry(model5_plan(float_class=True, rows=1), "A60")
        fns["A52_ms"] = entry(model5_plan(float_class=True, rows=2), "A52")
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    assert int(d_status.abs().sum().item()) == 0
    assert torch.equal(counts["A"], counts["B"]) and int(counts["A"][0].item()) == plan.targets_output_count(steps)
    if batch > POOL:
        assert torch.equal(audio["A"][:POOL].view(torch.int32), audio["A"][POOL: 2 * POOL].view(torch.int32))
    if float_class:
        assert torch.equal(audio["A60"].view(torch.int32), audio["A52"].view(torch.int32))
    med, spread = timed_alternating(fns, reps, 1)
    return dict(med, min_max=spread, reps=reps, batch=batch, float_class=float_class, steps_per_utterance=steps,
                samples_per_utterance=plan.targets_output_count(steps), points_per_utterance=points / POOL,
                # what an utterance reads: its points (8 bytes each) and 16 list ids, against 64 bytes per step
                input_bytes_per_utterance_A=points / POOL * 8 + 64, input_bytes_per_utterance_B=steps * 64,
                A_over_B=med["A_ms"] / med["B_ms"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", default="256,4096")
    ap.add_argument("--steps", type=int, default=60000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    results = []
    for float_class in (False, True):
        for batch in [int(b) for b in args.batches.split(",")]:
            results.append(measure(float_class, batch, args.steps, args.reps))
            print(json.dumps(results[-1]), flush=True)
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
