"""GPU-box: a targets session that keeps running (gvtm_stream_push_targets) beside the one route that exists
without it, on the same utterances.

Float plan of the male voice, SectionDelay 1, 4096 utterances in lockstep (a pool of 64 distinct ones tiled over the batch),
1200 internal steps as five pushes of 240, then finish.
  targets   the new entry: each push brings the points of its 240 steps (8 bytes a point), the filters run in the kernel
  frames    the parent's route for the same session: a stream of a plan whose control rate is its internal rate
            (control_steps == 1), fed gvtm_targets_apply_host's frames in the same five pieces (64 bytes a step)
Wall clock around the C calls alone (the tables of every push are packed beforehand), the two routes alternating inside every
repeat; mean and spread of the repeats after one warm-up session each, whose samples are compared byte for byte.
usage: python tests/tools/stream_targets_ab.py [--reps N] [--batch B] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import gama_tts_amd as g  # noqa: E402
from gama_tts_amd import capi  # noqa: E402
import stream_targets_cases as sessions  # noqa: E402
import targets_cases as cases  # noqa: E402
from voice_cases import male_plan  # noqa: E402

POOL, PUSHES, STEPS = 64, 5, 240


def tiled_tables(pool_lists, batch):
    """The tables of one push for `batch` utterances, utterance b given the 16 lists pool_lists[b % POOL]."""
    counts = np.array([len(l[0]) for u in pool_lists for l in u], dtype=np.int64)
    reps = -(-batch // len(pool_lists))
    offsets = np.zeros(16 * batch + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(np.tile(counts, reps)[: 16 * batch])
    _, steps, values = capi.pack_targets([l for u in pool_lists for l in u])
    assert batch % len(pool_lists) == 0
    return offsets, np.tile(steps, reps), np.tile(values, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    batch, total = args.batch, PUSHES * STEPS
    plan = male_plan(precision=capi.PRECISION_F32)
    rate = plan.info.internal_rate_hz
    today = male_plan(precision=capi.PRECISION_F32, crate=rate)
    assert today.info.control_steps == 1 and today.info.internal_rate_hz == rate
    lib, p = plan._lib, capi._ptr

    pool = [cases.spoken_lists(total, seed, stride=61) for seed in range(POOL)]
    pushes_new = [tiled_tables([sessions.slice_lists(u, i * STEPS, STEPS) for u in pool], batch) for i in range(PUSHES)]
    pool_frames = np.stack([capi.targets_apply_host(plan, u, total)[0] for u in pool])  # [POOL][total][16]
    pushes_old = [np.ascontiguousarray(np.tile(pool_frames[:, i * STEPS: (i + 1) * STEPS], (batch // POOL, 1, 1))) for i in range(PUSHES)]
    new, old = g.Stream(plan, batch), g.Stream(today, batch)
    stride = max(new.targets_capacity(STEPS), old.capacity(STEPS))
    audio, counts, maxabs = np.zeros((batch, stride), np.float32), np.zeros(batch, np.int64), np.zeros(batch, np.float32)

    def run(route, keep=None):
        """One session -> seconds per call (five pushes, finish); keep: a list that takes each call's samples of utterances 0 .. POOL."""
        stream = new if route == "targets" else old
        plan._check(lib.gvtm_stream_reset(stream._h))
        times = []
        for i in range(PUSHES + 1):
            t0 = time.perf_counter()
            if i == PUSHES:
                rc = lib.gvtm_stream_finish(stream._h, p(audio), stride, p(counts), p(maxabs))
            elif route == "targets":
                offsets, steps, values = pushes_new[i]
                rc = lib.gvtm_stream_push_targets(stream._h, p(offsets), p(steps), p(values), None, STEPS, p(audio), stride, p(counts), None)
            else:
                rc = lib.gvtm_stream_push(stream._h, p(pushes_old[i]), None, STEPS, p(audio), stride, p(counts))
            times.append(time.perf_counter() - t0)
            plan._check(rc)
            if keep is not None:
                keep.append([audio[b, : counts[b]].copy() for b in range(POOL)])
                if route == "targets":
                    held.append(int(new.targets_points().sum()))
        return times

    # warm-up, and the same bytes: per utterance the samples of the whole session, however the routes cut them into calls
    kept, held = {"targets": [], "frames": []}, [0]  # held[i]: the points the stream holds in front of push i, the whole batch's
    for route in kept:
        run(route, kept[route])
    for b in range(POOL):
        a, f = (np.concatenate([call[b] for call in kept[route]]) for route in ("targets", "frames"))
        assert a.size == plan.targets_output_count(total) and a.tobytes() == f.tobytes(), b

    times = {"targets": [], "frames": []}
    for _ in range(args.reps):
        for route in times:
            times[route].append(run(route))
    result = dict(batch=batch, steps=total, pushes=PUSHES, reps=args.reps, filter_length=plan.targets_filter_length(), same_bytes=True,
                  points_held_per_utterance_after_each_push=[h / batch for h in held[1: PUSHES + 1]])
    for route, runs in times.items():
        sums = [sum(r) for r in runs]
        result[route + "_session_ms"] = 1e3 * float(np.mean(sums))
        result[route + "_session_min_max_ms"] = [1e3 * min(sums), 1e3 * max(sums)]
        result[route + "_per_call_ms"] = [1e3 * float(x) for x in np.mean(np.asarray(runs), axis=0)]
    # host to device per push: the new route's log (what it held and the push's points, 8 bytes a point), list offsets and step
    # counts; the old one's frames (the look-ahead row with them) and frame counts
    result["targets_h2d_bytes_per_push_points"] = [8 * (held[i] + int(pushes_new[i][1].size)) for i in range(PUSHES)]
    result["targets_h2d_bytes_per_push_offsets_and_counts"] = 8 * (16 * batch + 1) + 4 * batch
    result["frames_h2d_bytes_per_push"] = 64 * batch * (STEPS + 1) + 4 * batch
    result["targets_over_frames"] = result["targets_session_ms"] / result["frames_session_ms"]
    print(json.dumps(result), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
