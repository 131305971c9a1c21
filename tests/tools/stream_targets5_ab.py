"""GPU-box: a model 5 targets session that keeps running (gvtm_stream_push_targets_model5) beside the only
model 5 session the parent commit has, and beside the one-shot entry, on the same utterances, in both classes.

5_male at 48 kHz (internal rate 60 411 Hz, filter of 3021 samples); utterances in lockstep (a pool of 16 distinct ones tiled
over the batch), 6000 internal steps as five pushes of 1200, then finish.
  A   the new entry: each push brings the points of its 1200 steps (8 bytes a point), the filters run in the kernel
  B   the parent's only model 5 session: gvtm_stream_push on a plan whose control rate is its internal rate
      (control_steps == 1), fed gvtm_targets_apply_host's frames in the same five pieces (64 bytes a step).  Its samples are
      NOT A's: it runs the model as the batch protocol constructs it, without the division by f0.  Time and bytes only
  C   one gvtm_synthesize_targets_model5_device call on the whole lists (tables on the device beforehand, shared through list
      ids), then the samples and counts copied to host memory as a session's are: what a session costs over a one-shot
Wall clock around the calls alone (the tables of every push are packed beforehand); three warm-up sessions of every route,
the routes alternating inside every repeat; median and [min, max] of the repeats.  Before anything is timed A's samples,
call by call, are compared byte for byte with C's.
usage: python tests/tools/stream_targets5_ab.py [--reps N] [--batches 256,4096] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import gama_tts_amd as g  # noqa: E402
from gama_tts_amd import capi  # noqa: E402
import stream_targets_cases as sessions  # noqa: E402
import targets_cases as cases  # noqa: E402
from stream_targets_ab import tiled_tables  # noqa: E402
from voice_cases import model5_plan  # noqa: E402

POOL, PUSHES, STEPS, WARMUPS = 16, 5, 1200, 3


def measure(float_class, batch, reps):
    total = PUSHES * STEPS
    plan = model5_plan(float_class=float_class)
    rate = plan.info.internal_rate_hz
    today = model5_plan(float_class=float_class, crate=rate)
    assert today.info.control_steps == 1 and today.info.internal_rate_hz == rate and batch % POOL == 0
    lib, p = plan._lib, capi._ptr
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731

    pool = [cases.spoken_lists(total, seed) for seed in range(POOL)]
    pushes_a = [tiled_tables([sessions.slice_lists(u, i * STEPS, STEPS) for u in pool], batch) for i in range(PUSHES)]
    pool_frames = np.stack([capi.targets_apply_host(plan, u, total)[0] for u in pool])  # [POOL][total][16]
    pushes_b = [np.ascontiguousarray(np.tile(pool_frames[:, i * STEPS: (i + 1) * STEPS], (batch // POOL, 1, 1))) for i in range(PUSHES)]
    a_stream, b_stream = g.Stream(plan, batch), g.Stream(today, batch)
    stride = max(a_stream.targets_capacity(STEPS), b_stream.capacity(STEPS))
    audio, counts, maxabs = np.zeros((batch, stride), np.float32), np.zeros(batch, np.int64), np.zeros(batch, np.float32)
    # C: the whole lists on the device, shared through list ids
    offsets, c_steps, c_values = capi.pack_targets([l for u in pool for l in u])
    ids = (np.arange(batch)[:, None] % POOL * 16 + np.arange(16)[None, :]).astype(np.int32)
    d_offsets, d_steps, d_values, d_ids = dev(offsets), dev(c_steps), dev(c_values), dev(ids)
    c_stride = plan.targets_output_capacity(total)
    d_audio, d_counts = torch.zeros((batch, c_stride), dtype=torch.float32, device="cuda"), torch.zeros(batch, dtype=torch.int64, device="cuda")
    d_status = torch.zeros(batch, dtype=torch.int32, device="cuda")
    hip_stream = torch.cuda.current_stream().cuda_stream

    def run(route, keep=None):
        """One session (C: one call and its copies) -> seconds; keep: a list that takes each call's samples of utterances 0 .. POOL."""
        if route == "C":
            t0 = time.perf_counter()
            plan.synthesize_targets_model5_device(d_offsets, POOL * 16, d_ids, d_steps, d_values, None, batch, total, d_audio, c_stride, d_counts, None,
                                                  d_status, hip_stream)
            host_audio, host_counts = d_audio.cpu(), d_counts.cpu()
            seconds = time.perf_counter() - t0
            if keep is not None:
                keep.append([host_audio[b, : int(host_counts[b])].numpy().copy() for b in range(POOL)])
            return seconds
        stream = a_stream if route == "A" else b_stream
        plan._check(lib.gvtm_stream_reset(stream._h))
        seconds = 0.0
        for i in range(PUSHES + 1):
            t0 = time.perf_counter()
            if i == PUSHES:
                rc = lib.gvtm_stream_finish(stream._h, p(audio), stride, p(counts), p(maxabs))
            elif route == "A":
                tables = pushes_a[i]
                rc = lib.gvtm_stream_push_targets_model5(stream._h, p(tables[0]), p(tables[1]), p(tables[2]), None, STEPS, p(audio), stride, p(counts), None)
            else:
                rc = lib.gvtm_stream_push(stream._h, p(pushes_b[i]), None, STEPS, p(audio), stride, p(counts))
            seconds += time.perf_counter() - t0
            plan._check(rc)
            if keep is not None:
                keep.append([audio[b, : counts[b]].copy() for b in range(POOL)])
        return seconds

    kept = {"A": [], "B": [], "C": []}
    for route in kept:
        run(route, kept[route])
    assert int(d_status.abs().sum().item()) == 0
    differ = 0
    for b in range(POOL):
        a, c = np.concatenate([call[b] for call in kept["A"]]), kept["C"][0][b]
        old = np.concatenate([call[b] for call in kept["B"]])
        assert a.size == plan.targets_output_count(total) == old.size and a.tobytes() == c.tobytes(), b
        differ += a.tobytes() != old.tobytes()
    assert differ == POOL  # (B is another model: no utterance has A's samples)
    for _ in range(WARMUPS - 1):
        for route in kept:
            run(route)
    times = {route: [] for route in kept}
    for _ in range(reps):
        for route in times:
            times[route].append(run(route))
    points = [int(t[1].size) // batch for t in pushes_a]
    result = dict(float_class=float_class, batch=batch, steps=total, pushes=PUSHES, reps=reps, filter_length=plan.targets_filter_length(),
                  A_equals_C=True, B_differs=True, points_per_utterance_per_push=points,
                  # host to device per push and utterance: A the log (at most the points of the last N + 12 steps and one per list, with
                  # the push's own; 8 bytes each) and 17 offsets; B the frames with the look-ahead row
                  B_h2d_bytes_per_utterance_per_push=64 * (STEPS + 1) + 4)
    for route, runs in times.items():
        result[route + "_ms"] = 1e3 * float(np.median(runs))
        result[route + "_min_max_ms"] = [1e3 * min(runs), 1e3 * max(runs)]
    result["A_over_B"] = result["A_ms"] / result["B_ms"]
    result["A_over_C"] = result["A_ms"] / result["C_ms"]
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", default="256,4096")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    results = []
    for float_class in (False, True):
        for batch in [int(b) for b in args.batches.split(",")]:
            results.append(measure(float_class, batch, args.reps))
            print(json.dumps(results[-1]), flush=True)
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
