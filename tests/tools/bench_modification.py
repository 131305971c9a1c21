"""GPU-box: parameter-modification gestures applied to frames on the device (gvtm_apply_modifications_device)
beside the synthesis launch of the same batch.

Utterances over one shared base, float plan of the male voice, one ADD gesture on r3 each, everything resident:
  one      1 point: the walk's jump takes it from the point's entry (the first step) to the end
  fifty    50 points spread over the utterance: N steps and one per point
  half_n   a point every N / 2 steps: the entering and the leaving value never agree, every step is walked
  synth    gvtm_synthesize_batch_device on the frames the last apply left (the parent's kernel, unchanged)
Three workloads: 4096 utterances x 500 frames at SectionDelay 1, (fifty, half_n) 512 utterances of the same, and (one,
half_n) 512 utterances x 7500 frames at SectionDelay 2.  The variants alternate inside every repeat; medians, wall time between HIP events after warm-up.  Before
anything is timed the device's frames are compared with gvtm_modification_apply_host's on a few utterances of every variant.
usage: python tests/tools/bench_modification.py [--reps N] [--small] [--out FILE.json]"""
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
from bench_tracks_voices import timed_alternating  # noqa: E402
from voice_cases import configs  # noqa: E402

R3 = 9
APPLY_CALLS = 10  # per timed window


def gestures_of(kind, batch, frames, cs, n):
    """One ADD gesture on r3 per utterance -> per utterance (steps, values); the steps differ a little between utterances."""
    end = (frames - 1) * cs
    out = []
    for b in range(batch):
        rng = np.random.default_rng([b, frames])
        if kind == "one":
            steps = np.array([3 * cs + b % cs])
        elif kind == "fifty":
            steps = np.sort(rng.choice(np.arange(end), 50, replace=False))
        else:
            steps = np.arange(b % 7, end, n // 2)
        out.append((steps.astype(np.int32), rng.uniform(-0.1, 0.1, steps.size).astype(np.float32)))
    return out


def workload(delay, batch, frames, kinds, reps, results):
    stream = torch.cuda.current_stream().cuda_stream
    plan = g.Plan(configs(44100.0, delay, capi.PRECISION_F32, names=["male"])[0], 250.0, 0)
    cs, n = plan.info.control_steps, plan.modification_filter_length()
    base = tracks.random_track(frames, 4242, consonant_heavy=True)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    d_base, d_base_counts = dev(base[None]), dev(np.array([frames], np.int32))
    d_ids = torch.zeros(batch, dtype=torch.int32, device="cuda")
    d_params = torch.zeros((batch, frames, 16), dtype=torch.float32, device="cuda")
    d_counts = torch.zeros(batch, dtype=torch.int32, device="cuda")
    d_status = torch.zeros(batch, dtype=torch.int32, device="cuda")
    stride = plan.output_capacity(frames)
    d_audio = torch.zeros((batch, stride), dtype=torch.float32, device="cuda")
    d_out_counts = torch.zeros(batch, dtype=torch.int64, device="cuda")
    plan.reserve(frames)
    tables, points = {}, {}
    for kind in kinds:
        per = gestures_of(kind, batch, frames, cs, n)
        table, offsets, utt, steps, values = capi.pack_gestures([[(R3, 0, s, v)] for s, v in per])
        tables[kind] = tuple(dev(x) for x in (table, offsets, utt, steps, values))
        points[kind] = int(steps.size)

        def apply(kind=kind):
            t = tables[kind]
            plan.apply_modifications_device(d_base, d_base_counts, 1, d_ids, t[0], t[1], t[2], t[3], t[4], None, batch, frames, d_params, d_counts,
                                            d_status, stream)
        apply()
        torch.cuda.synchronize()
        assert int(d_status.abs().sum().item()) == 0 and int(d_counts.min().item()) == frames
        for b in sorted({0, 1, batch // 2, batch - 1}):
            want, status = capi.modification_apply_host(plan, base, [(R3, 0) + per[b]])
            assert status == 0 and d_params[b].cpu().numpy().tobytes() == want.tobytes(), (kind, b)
        tables[kind + "_fn"] = apply

    def synth():
        plan.synthesize_device(d_params, batch, frames, d_audio, stride, d_counts, d_out_counts, None, stream)

    def ten_times(fn):
        return lambda: [fn() for _ in range(APPLY_CALLS)]

    fns = {kind + "_ms": ten_times(tables[kind + "_fn"]) for kind in kinds}  # (an apply call is short: ten per timed window)
    fns["synth_ms"] = synth
    med, spread = timed_alternating(fns, reps, 1)
    for key in med:
        if key != "synth_ms":
            med[key], spread[key] = med[key] / APPLY_CALLS, [t / APPLY_CALLS for t in spread[key]]
    name = "delay%d_%dx%d" % (delay, batch, frames)
    results[name] = dict(med, min_max=spread, control_steps=cs, filter_length=n, steps_per_utterance=(frames - 1) * cs, points_total=points,
                         device_frames_equal_host_frames=True,
                         **{kind + "_over_synth": med[kind + "_ms"] / med["synth_ms"] for kind in kinds})
    if "half_n" in kinds:  # every step walked, one lane per utterance: the dependent chain's cost per step
        results[name]["half_n_ns_per_step"] = med["half_n_ms"] * 1e6 / ((frames - 1) * cs)
    print(json.dumps({name: results[name]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="an eighth of the utterances (a quick look)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    shrink = 8 if args.small else 1
    results = {"reps": args.reps}
    workload(1, 4096 // shrink, 500, ("one", "fifty", "half_n"), args.reps, results)
    # the same utterances, an eighth as many wavefronts (four per SIMD against half a one): what the chain costs per step by itself
    workload(1, 512 // shrink, 500, ("fifty", "half_n"), args.reps, results)
    workload(2, 512 // shrink, 7500, ("one", "half_n"), args.reps, results)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
