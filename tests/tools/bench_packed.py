"""GPU-box: a ragged batch through the padded host entry against the packed one (include/gama_vtm.h, "Ragged batches").

4096 utterances on the float plan of the male voice (SectionDelay 1, 44.1 kHz), frame counts uniform in [50, 500] from a
fixed seed, page-locked buffers, int16 out.  Wall time per synchronous call of
  padded   gvtm_synthesize_batch_host_pcm16: [batch][max frames][16] in, [batch][stride] out, frame counts beside them
  packed   gvtm_synthesize_packed_host_pcm16: the frames back to back in, the samples back to back out
each in the caller's (random) order and with the utterances sorted by length, with the bytes each call moves each way and
the device time of its synthesis launches (gvtm_plan_set_timing).  Every variant is warmed up first; the repeats then
alternate the variants, so that what else the machine does falls on all of them alike.  Per variant: the median, the
fastest and the slowest repeat and spread = (slowest - fastest) / median.
usage: python tests/tools/bench_packed.py [--reps N] [--batch B] [--min-frames A] [--max-frames Z] [--out FILE.json]"""
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
import tracks  # noqa: E402
from voice_cases import male_plan  # noqa: E402


def build(plan, pool, frame_counts):
    """Page-locked buffers of both layouts for these utterances (utterance b: the first frame_counts[b] frames of pool track
    b % len(pool)) -> dict of the two calls and what they move."""
    batch, longest = len(frame_counts), int(frame_counts.max())
    stride = plan.output_capacity(longest)
    fo = np.zeros(batch + 1, np.int64)
    fo[1:] = np.cumsum(frame_counts)
    offsets = plan.packed_sample_offsets(fo)
    pin = dict(padded_in=g.PinnedArray((batch, longest, 16), np.float32), padded_out=g.PinnedArray((batch, stride), np.int16),
               packed_in=g.PinnedArray((int(fo[batch]), 16), np.float32), packed_out=g.PinnedArray((int(offsets[batch]),), np.int16))
    pin["padded_in"].array[...] = 0.0
    for b, f in enumerate(frame_counts):
        track = pool[b % len(pool), :f]
        pin["padded_in"].array[b, :f] = track
        pin["packed_in"].array[fo[b]: fo[b + 1]] = track
    fc = frame_counts.astype(np.int32)
    counts = [np.zeros(batch, np.int64) for _ in range(2)]
    maxabs = [np.zeros(batch, np.float32) for _ in range(2)]
    scales = [np.zeros(batch, np.float32) for _ in range(2)]

    def padded():
        plan.synthesize_host_into(pin["padded_in"].array, pin["padded_out"].array, fc, counts[0], maxabs[0], scales[0])

    def packed():
        plan.synthesize_packed_host_into(pin["packed_in"].array, fo, pin["packed_out"].array, None, None, counts[1], maxabs[1], scales[1])

    def same():
        """the two calls' results, utterance by utterance"""
        ok = np.array_equal(counts[0], counts[1]) and np.array_equal(maxabs[0], maxabs[1]) and np.array_equal(scales[0], scales[1])
        for b in range(batch):
            n = int(counts[0][b])
            ok = ok and np.array_equal(pin["padded_out"].array[b, :n], pin["packed_out"].array[offsets[b]: offsets[b] + n])
        return bool(ok)

    moved = {"padded": {"h2d_bytes": int(batch * longest * 64 + 4 * batch), "d2h_bytes": int(batch * stride * 2)},
             "packed": {"h2d_bytes": int(fo[batch] * 64 + 16 * (batch + 1)), "d2h_bytes": int(offsets[batch] * 2)}}
    return {"padded": padded, "packed": packed, "same": same, "moved": moved, "pin": pin}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--min-frames", type=int, default=50)
    ap.add_argument("--max-frames", type=int, default=500)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 5:
        sys.exit("at least five repeats per variant")
    plan = male_plan(precision=capi.PRECISION_F32)
    rng = np.random.default_rng(20240)
    frame_counts = rng.integers(args.min_frames, args.max_frames + 1, size=args.batch)
    pool = tracks.random_tracks(64, args.max_frames, seed0=1000, consonant_heavy=True)
    orders = {"caller": build(plan, pool, frame_counts), "sorted": build(plan, pool, np.sort(frame_counts))}
    fns = {"%s_%s" % (kind, order): orders[order][kind] for order in orders for kind in ("padded", "packed")}
    plan.set_timing(True)
    kernel_ms = {}
    for name, fn in fns.items():  # warm-up, and the device time of each variant's synthesis launches
        fn()
        plan.take_kernel_ms()
        fn()
        ms, launches = plan.take_kernel_ms()
        kernel_ms[name] = {"synthesis_launches": launches, "synthesis_ms_sum": ms * launches}
    plan.set_timing(False)
    stats = plan.packed_stats()
    identical = {order: orders[order]["same"]() for order in orders}
    times = {name: [] for name in fns}
    for _ in range(args.reps):
        for name, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
    result = {"batch": args.batch, "frames": [args.min_frames, args.max_frames], "mean_frames": float(frame_counts.mean()), "reps": args.reps,
              "output": "int16", "precision": "float", "packed_equals_padded": identical,
              "packed_staging_bytes": int(stats.staging_bytes), "packed_slices_last_call": int(stats.slices), "variants": {}}
    for name in fns:
        kind, order = name.split("_")
        t = np.array(times[name])
        row = {"ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max()), "spread": float((t.max() - t.min()) / np.median(t))}
        row.update(orders[order]["moved"][kind])
        row.update(kernel_ms[name])
        row["d2h_gb_per_s_of_wall"] = row["d2h_bytes"] / row["ms"] / 1e6
        result["variants"][name] = row
    for order in orders:
        result["padded_over_packed_" + order] = result["variants"]["padded_" + order]["ms"] / result["variants"]["packed_" + order]["ms"]
    print(json.dumps(result), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    for order in orders.values():
        for p in order["pin"].values():
            p.close()


if __name__ == "__main__":
    main()
