"""GPU-box: synthesis from parameter targets (gvtm_synthesize_targets_device) beside the two routes that exist
without it, on the same utterances.

Float plan of the male voice, SectionDelay 1, utterances of 1 s of internal steps (250 frames' worth: 20 000), about 20 points
per parameter, a pool of 64 distinct utterances tiled over the batch (through list ids: the pool's lists are shared).
  targets   the new entry: the points in, the filter in the synthesis kernel's interpolation wavefront
  A         today's route to the same samples: a plan whose control rate is its internal rate (control_steps == 1) and the
            per-step frames of gvtm_targets_apply_host already resident in device memory (64 bytes per step and utterance)
  B         the ordinary launch at 250 Hz of the same number of steps (other samples: frames interpolated linearly)
The three alternate inside every repeat; medians and the spread of the repeats, wall time between HIP events after warm-up.
Before anything is timed the new entry's samples are compared with A's, byte for byte, over the whole batch.
usage: python tests/tools/targets_ab.py [--reps N] [--batch B] [--out FILE.json]"""
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
import tracks  # noqa: E402
from bench_tracks_voices import timed_alternating  # noqa: E402
from voice_cases import male_plan  # noqa: E402

POOL, FRAMES = 64, 250


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    batch = args.batch
    stream = torch.cuda.current_stream().cuda_stream
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    plan = male_plan(precision=capi.PRECISION_F32)
    rate, cs = plan.info.internal_rate_hz, plan.info.control_steps
    steps = FRAMES * cs
    today = male_plan(precision=capi.PRECISION_F32, crate=rate)
    assert today.info.control_steps == 1 and today.info.internal_rate_hz == rate
    stride = plan.targets_output_capacity(steps)
    assert stride == today.output_capacity(steps) == plan.output_capacity(FRAMES)

    # the pool: 16 lists per utterance, a point every steps / 20 steps or so; and its frames by the host rule
    pool = [cases.spoken_lists(steps, seed, stride=steps // 20 + 7) for seed in range(POOL)]
    points = sum(len(l[0]) for u in pool for l in u)
    offsets, p_steps, p_values = capi.pack_targets([l for u in pool for l in u])
    ids = (np.arange(batch)[:, None] % POOL * 16 + np.arange(16)[None, :]).astype(np.int32)
    d_offsets, d_steps, d_values, d_ids = dev(offsets), dev(p_steps), dev(p_values), dev(ids)
    pool_frames = np.stack([capi.targets_apply_host(plan, u, steps)[0] for u in pool])
    d_frames_a = dev(pool_frames)[torch.arange(batch, device="cuda") % POOL].contiguous()  # [batch][steps][16]: 64 bytes per step
    d_frames_b = dev(tracks.random_tracks(POOL, FRAMES, seed0=7, consonant_heavy=True))[torch.arange(batch, device="cuda") % POOL].contiguous()
    audio = {k: torch.zeros((batch, stride), dtype=torch.float32, device="cuda") for k in ("targets", "A", "B")}
    counts = {k: torch.zeros(batch, dtype=torch.int64, device="cuda") for k in audio}
    d_status = torch.zeros(batch, dtype=torch.int32, device="cuda")
    plan.reserve(FRAMES)
    today.reserve(steps)

    fns = {
        "targets_ms": lambda: plan.synthesize_targets_device(d_offsets, POOL * 16, d_ids, d_steps, d_values, None, batch, steps, audio["targets"], stride,
                                                             counts["targets"], None, d_status, stream),
        "A_ms": lambda: today.synthesize_device(d_frames_a, batch, steps, audio["A"], stride, None, counts["A"], None, stream),
        "B_ms": lambda: plan.synthesize_device(d_frames_b, batch, FRAMES, audio["B"], stride, None, counts["B"], None, stream),
    }
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    assert int(d_status.abs().sum().item()) == 0
    assert torch.equal(counts["targets"], counts["A"]) and torch.equal(counts["A"], counts["B"])
    assert torch.equal(audio["targets"].view(torch.int32), audio["A"].view(torch.int32))
    med, spread = timed_alternating(fns, args.reps, 1)
    results = dict(med, min_max=spread, reps=args.reps, batch=batch, steps_per_utterance=steps, filter_length=plan.targets_filter_length(),
                   points_per_utterance=points / POOL, point_bytes_per_utterance=8 * points / POOL, frame_bytes_per_utterance_A=64 * steps,
                   samples_per_utterance=int(counts["A"][0].item()), targets_equal_A_bytes=True,
                   targets_over_A=med["targets_ms"] / med["A_ms"], targets_over_B=med["targets_ms"] / med["B_ms"])
    print(json.dumps(results), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
