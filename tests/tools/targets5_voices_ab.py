"""GPU-box: model 5 parameter targets under a mix of voices in one launch (gvtm_synthesize_targets_model5_voices_device;
DESIGN.md 6e) beside the route that exists without it, on the same utterances, in both classes.

The five 5_male voices at 48 kHz (internal rates 60.4 to 141 kHz, filters of 3021 to 7048 samples); utterances of --steps
internal steps, about 20 points per parameter, a pool of 16 distinct utterances tiled over the batch through list ids.
  A   the new entry: one plan of the five voices, the voice ids spread evenly and interleaved (utterance b: voice b mod 5)
  B   without it: five one-voice plans and five gvtm_synthesize_targets_model5_device launches of a fifth of the batch each,
      one after another on one stream, from the first enqueue to the last completion
  V   an entry that existed before, for a before / after of its own: gvtm_synthesize_voices_device on the same five-voice
      plan, frames at 250 Hz (--frames of them per utterance, random tracks, the same ids)
The routes alternate inside every repeat; medians and the spread of the repeats, time between HIP events after warm-up.
Before anything is timed A's rows are compared with B's, byte for byte, over the whole batch.
--existing-only times V alone, which a library from before the entry can run too (GVTM_LIBRARY names it).
usage: python tests/tools/targets5_voices_ab.py [--reps N] [--batches 256,4096] [--steps S] [--frames F] [--existing-only] [--out FILE.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
from gama_tts_amd import capi  # noqa: E402
import targets5_voices_cases as v5  # noqa: E402
import targets_cases as cases  # noqa: E402
import tracks  # noqa: E402
from bench_tracks_voices import timed_alternating  # noqa: E402
from voice_files import VOICES  # noqa: E402

POOL = 16


def measure(float_class, batch, steps, frames, reps, existing_only):
    stream = torch.cuda.current_stream().cuda_stream
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    n_voices = len(VOICES)
    plan = v5.voices_plan(float_class, device=0)
    voice_ids = (np.arange(batch) % n_voices).astype(np.int32)
    d_voices = dev(voice_ids)
    fns = {}

    # V: frames under the five voices (gvtm_synthesize_voices_device)
    pool_frames = tracks.random_tracks(POOL, frames, seed0=7, consonant_heavy=True)
    d_params = dev(pool_frames).repeat((batch + POOL - 1) // POOL, 1, 1)[:batch].contiguous()
    stride_v = plan.voices_output_capacity(frames)
    audio_v = torch.zeros((batch, stride_v), dtype=torch.float32, device="cuda")
    counts_v = torch.zeros(batch, dtype=torch.int64, device="cuda")
    fns["V_ms"] = lambda: plan.synthesize_voices_device(d_params, d_voices, batch, frames, audio_v, stride_v, None, counts_v, None, stream)

    if not existing_only:
        singles = [v5.single_plan(float_class, name, device=0) for name in VOICES]
        stride = plan.targets_voices_output_capacity(steps)
        pool = [cases.spoken_lists(steps, seed, stride=steps // 20 + 7) for seed in range(POOL)]
        points = sum(len(l[0]) for u in pool for l in u)
        offsets, p_steps, p_values = capi.pack_targets([l for u in pool for l in u])
        ids = (np.arange(batch)[:, None] % POOL * 16 + np.arange(16)[None, :]).astype(np.int32)
        d_offsets, d_steps, d_values, d_ids = dev(offsets), dev(p_steps), dev(p_values), dev(ids)
        # B: voice v's utterances in batch order, their list ids back to back
        of_voice = [np.nonzero(voice_ids == v)[0] for v in range(n_voices)]
        d_ids_b = [dev(ids[rows]) for rows in of_voice]
        audio_a = torch.zeros((batch, stride), dtype=torch.float32, device="cuda")
        audio_b = [torch.zeros((len(rows), stride), dtype=torch.float32, device="cuda") for rows in of_voice]
        counts_a = torch.zeros(batch, dtype=torch.int64, device="cuda")
        counts_b = [torch.zeros(len(rows), dtype=torch.int64, device="cuda") for rows in of_voice]
        d_status = torch.zeros(batch, dtype=torch.int32, device="cuda")

        def route_b():
            for v, single in enumerate(singles):
                single.synthesize_targets_model5_device(d_offsets, POOL * 16, d_ids_b[v], d_steps, d_values, None, len(of_voice[v]), steps, audio_b[v],
                                                        stride, counts_b[v], None, None, stream)

        fns["A_ms"] = lambda: plan.synthesize_targets_model5_voices_device(d_offsets, POOL * 16, d_ids, d_steps, d_values, None, d_voices, batch, steps,
                                                                           audio_a, stride, counts_a, None, d_status, stream)
        fns["B_ms"] = route_b
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    results = dict(reps=reps, batch=batch, float_class=float_class, frames_per_utterance_V=frames)
    if not existing_only:
        assert int(d_status.abs().sum().item()) == 0
        for v, rows in enumerate(of_voice):
            idx = torch.from_numpy(rows).cuda()
            assert torch.equal(counts_a[idx], counts_b[v]), v
            assert torch.equal(audio_a[idx].view(torch.int32), audio_b[v].view(torch.int32)), v
        results.update(steps_per_utterance=steps, points_per_utterance=points / POOL, A_equals_B_bytes=True,
                       filter_lengths=[plan.targets_filter_length(v) for v in range(n_voices)],
                       samples_per_utterance_by_voice=[plan.targets_voice_output_count(v, steps) for v in range(n_voices)])
    med, spread = timed_alternating(fns, reps, 1)
    results.update(med, min_max=spread)
    if not existing_only:
        results["A_over_B"] = med["A_ms"] / med["B_ms"]
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", default="256,4096")
    ap.add_argument("--steps", type=int, default=30000)
    ap.add_argument("--frames", type=int, default=125)
    ap.add_argument("--existing-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    results = []
    for float_class in (False, True):
        for batch in [int(b) for b in args.batches.split(",")]:
            results.append(measure(float_class, batch, args.steps, args.frames, args.reps, args.existing_only))
            print(json.dumps(results[-1]), flush=True)
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
