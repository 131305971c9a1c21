"""GPU-box: a targets session under a mix of voices on ONE stream (gvtm_stream_push_targets_voices,
gvtm_stream_push_targets_model5_voices) beside what the parent commit offers for the same utterances, and
beside the one-shot voices entry, in both model families.

Utterance b is spoken by voice b mod V and walks the lists of a pool of 16 distinct utterances (b mod 16); 6000 internal steps
as five pushes of 1200, then finish.
  A   the new entry: one stream of the plan of V voices, one launch a push
  B   the parent's route: V one-voice plans with a stream each, voice v's utterances (in their batch order) pushed into
      stream v with the existing one-voice entry, the V streams in turn -- V launches a push, each on a fifth (a quarter) of
      the batch.  Its samples are A's byte for byte (asserted before anything is timed, every utterance)
  C   one one-shot voices call on the whole lists (tables on the device beforehand, shared through list ids), then the
      samples and counts copied to host memory as a session's are: what a session costs over a one-shot
Families: model 5 in both classes with its five voices; the models 0 to 4 in float with the four voices that up-sample at
44.1 kHz, and with the baby voice (which down-samples) added.
Wall clock around the calls alone (the tables of every push are packed beforehand); three warm-up sessions of every route,
the routes alternating inside every repeat; median and [min, max] of the repeats.  No ratio is a pass condition.
usage: python tests/tools/stream_targets_voices_ab.py [--reps N] [--batches 256,4096] [--families a,b] [--out FILE.json]"""
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
import targets5_voices_cases as cases5  # noqa: E402
import targets_cases as cases  # noqa: E402
from voice_cases import configs  # noqa: E402
from voice_files import VOICES  # noqa: E402

POOL, PUSHES, STEPS, WARMUPS = 16, 5, 1200, 3
UP4 = ["male", "female", "large_child", "small_child"]
FAMILIES = ["model5-double", "model5-float", "float-up4", "float-with-baby"]


def plans_of(family):
    """-> (the plan of V voices, the V one-voice plans, model 5?)"""
    if family.startswith("model5"):
        float_class = family == "model5-float"
        return cases5.voices_plan(float_class, device=0), [cases5.single_plan(float_class, name, device=0) for name in VOICES], True
    names = UP4 if family == "float-up4" else list(VOICES)
    cfgs = configs(44100.0, 1, capi.PRECISION_F32, names=names)
    return g.VoicesPlan(cfgs, 250.0, 0), [g.Plan(cfg, 250.0, 0) for cfg in cfgs], False


def tables_of(pool_pieces, utterances):
    """The tables of one push for the utterances `utterances` (batch indices), utterance b given the lists pool_pieces[b % POOL]."""
    return capi.pack_targets([l for b in utterances for l in pool_pieces[b % POOL]])


def measure(family, batch, reps):
    total = PUSHES * STEPS
    plan, singles, model5 = plans_of(family)
    V = len(singles)
    lib, p = plan._lib, capi._ptr
    push_a = lib.gvtm_stream_push_targets_model5_voices if model5 else lib.gvtm_stream_push_targets_voices
    push_b = lib.gvtm_stream_push_targets_model5 if model5 else lib.gvtm_stream_push_targets
    one_shot = plan.synthesize_targets_model5_voices_device if model5 else plan.synthesize_targets_voices_device
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    ids = (np.arange(batch) % V).astype(np.int32)
    mine = [[b for b in range(batch) if ids[b] == v] for v in range(V)]

    pool = [cases.spoken_lists(total, seed) for seed in range(POOL)]
    pieces = [[sessions.slice_lists(u, i * STEPS, STEPS) for u in pool] for i in range(PUSHES)]
    pushes_a = [tables_of(pieces[i], range(batch)) for i in range(PUSHES)]
    pushes_b = [[tables_of(pieces[i], mine[v]) for v in range(V)] for i in range(PUSHES)]
    a_stream = g.Stream(plan, batch, voice_ids=ids)
    b_streams = [g.Stream(singles[v], len(mine[v])) for v in range(V)]
    stride = a_stream.targets_capacity(STEPS)
    audio, counts, maxabs = np.zeros((batch, stride), np.float32), np.zeros(batch, np.int64), np.zeros(batch, np.float32)
    b_strides = [s.targets_capacity(STEPS) for s in b_streams]
    b_audio = [np.zeros((len(mine[v]), b_strides[v]), np.float32) for v in range(V)]
    b_counts, b_maxabs = [np.zeros(len(m), np.int64) for m in mine], [np.zeros(len(m), np.float32) for m in mine]
    # C: the whole lists on the device, shared through list ids
    offsets, c_steps, c_values = capi.pack_targets([l for u in pool for l in u])
    list_ids = (np.arange(batch)[:, None] % POOL * 16 + np.arange(16)[None, :]).astype(np.int32)
    d_offsets, d_steps, d_values, d_ids, d_voices = dev(offsets), dev(c_steps), dev(c_values), dev(list_ids), dev(ids)
    c_stride = plan.targets_voices_output_capacity(total)
    d_audio, d_counts = torch.zeros((batch, c_stride), dtype=torch.float32, device="cuda"), torch.zeros(batch, dtype=torch.int64, device="cuda")
    d_status = torch.zeros(batch, dtype=torch.int32, device="cuda")
    hip_stream = torch.cuda.current_stream().cuda_stream

    def run(route, keep=None):
        """One session (C: one call and its copies) -> seconds; keep: a dict that takes every utterance's samples, call by call."""
        if route == "C":
            t0 = time.perf_counter()
            one_shot(d_offsets, POOL * 16, d_ids, d_steps, d_values, None, d_voices, batch, total, d_audio, c_stride, d_counts, None, d_status, hip_stream)
            host_audio, host_counts = d_audio.cpu(), d_counts.cpu()
            seconds = time.perf_counter() - t0
            if keep is not None:
                for b in range(batch):
                    keep[b] = [host_audio[b, : int(host_counts[b])].numpy().copy()]
            return seconds
        if route == "A":
            plan._check(lib.gvtm_stream_reset(a_stream._h))
        else:
            for v in range(V):
                plan._check(lib.gvtm_stream_reset(b_streams[v]._h))
        seconds = 0.0
        for i in range(PUSHES + 1):
            t0 = time.perf_counter()
            if route == "A":
                if i == PUSHES:
                    rc = lib.gvtm_stream_finish(a_stream._h, p(audio), stride, p(counts), p(maxabs))
                else:
                    t = pushes_a[i]
                    rc = push_a(a_stream._h, p(t[0]), p(t[1]), p(t[2]), None, STEPS, p(audio), stride, p(counts), None)
            else:
                rc = 0
                for v in range(V):
                    if rc:
                        break
                    if i == PUSHES:
                        rc = lib.gvtm_stream_finish(b_streams[v]._h, p(b_audio[v]), b_strides[v], p(b_counts[v]), p(b_maxabs[v]))
                    else:
                        t = pushes_b[i][v]
                        rc = push_b(b_streams[v]._h, p(t[0]), p(t[1]), p(t[2]), None, STEPS, p(b_audio[v]), b_strides[v], p(b_counts[v]), None)
            seconds += time.perf_counter() - t0
            plan._check(rc)
            if keep is not None:
                for b in range(batch):
                    if route == "A":
                        keep.setdefault(b, []).append(audio[b, : counts[b]].copy())
                    else:
                        v, j = int(ids[b]), b // V
                        keep.setdefault(b, []).append(b_audio[v][j, : b_counts[v][j]].copy())
        return seconds

    kept = {"A": {}, "B": {}, "C": {}}
    for route in kept:
        run(route, kept[route])
    assert int(d_status.abs().sum().item()) == 0
    for b in range(batch):
        a = np.concatenate(kept["A"][b]).tobytes()
        assert len(a) == 4 * plan.targets_voice_output_count(int(ids[b]), total), b
        assert a == np.concatenate(kept["B"][b]).tobytes(), ("A != B", b)
        assert a == kept["C"][b][0].tobytes(), ("A != C", b)
    kept = None
    for _ in range(WARMUPS - 1):
        for route in "ABC":
            run(route)
    times = {route: [] for route in "ABC"}
    for _ in range(reps):
        for route in times:
            times[route].append(run(route))
    result = dict(family=family, batch=batch, voices=V, steps=total, pushes=PUSHES, reps=reps,
                  filter_lengths=[plan.targets_filter_length(v) for v in range(V)], A_equals_B=True, A_equals_C=True)
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
    ap.add_argument("--families", default=",".join(FAMILIES))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    results = []
    for family in args.families.split(","):
        for batch in [int(b) for b in args.batches.split(",")]:
            results.append(measure(family, batch, args.reps))
            print(json.dumps(results[-1]), flush=True)
            torch.cuda.empty_cache()
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as f:
                    json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
