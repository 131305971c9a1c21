"""GPU-box: parameter targets under a mix of voices in one launch (gvtm_synthesize_targets_voices_device) beside
the route that exists without it, on the same utterances.

Float plans, SectionDelay 1, 44.1 kHz; utterances of 20 000 internal steps, about 20 points per parameter, a pool of 64
distinct utterances tiled over the batch through list ids (the workload of targets_ab.py).
  A   the new entry: one plan of the five voices, the voice ids spread evenly and interleaved (utterance b: voice b mod 5)
  B   without it: five one-voice plans and five gvtm_synthesize_targets_device launches of a fifth of the batch each, one
      after another on one stream, from the first enqueue to the last completion
  C   the one-voice entry on the whole batch under the male voice: what the mix of voices costs
The three alternate inside every repeat; medians and the spread of the repeats, time between HIP events after warm-up.
Before anything is timed A's rows are compared with B's, byte for byte, over the whole batch.
--voices picks the plan's voices: a plan with the baby voice, whose internal rate lies above 44.1 kHz, launches two rows per
workgroup and the reference's 1024-sample rings for every voice; without it the mix launches the four rows of route C.
usage: python tests/tools/targets_voices_ab.py [--reps N] [--batch B] [--voices a,b,..] [--out FILE.json]"""
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
import targets_cases as cases  # noqa: E402
from bench_tracks_voices import timed_alternating  # noqa: E402
from voice_cases import configs  # noqa: E402
from voice_files import VOICES  # noqa: E402

POOL, STEPS = 64, 20000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--voices", default=None, help="comma-separated voice names (default: all five)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    batch = args.batch
    stream = torch.cuda.current_stream().cuda_stream
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    names = args.voices.split(",") if args.voices else list(VOICES)
    cfgs = configs(44100.0, 1, capi.PRECISION_F32, names=names)
    n_voices = len(cfgs)
    plan = g.VoicesPlan(cfgs, 250.0, 0)
    singles = [g.Plan(c, 250.0, 0) for c in cfgs]
    stride = plan.targets_voices_output_capacity(STEPS)

    pool = [cases.spoken_lists(STEPS, seed, stride=STEPS // 20 + 7) for seed in range(POOL)]
    points = sum(len(l[0]) for u in pool for l in u)
    offsets, p_steps, p_values = capi.pack_targets([l for u in pool for l in u])
    ids = (np.arange(batch)[:, None] % POOL * 16 + np.arange(16)[None, :]).astype(np.int32)
    voice_ids = (np.arange(batch) % n_voices).astype(np.int32)
    d_offsets, d_steps, d_values, d_ids, d_voices = dev(offsets), dev(p_steps), dev(p_values), dev(ids), dev(voice_ids)
    # B: voice v's utterances in batch order, their list ids back to back
    of_voice = [np.nonzero(voice_ids == v)[0] for v in range(n_voices)]
    d_ids_b = [dev(ids[rows]) for rows in of_voice]
    audio = {k: torch.zeros((batch, stride), dtype=torch.float32, device="cuda") for k in ("A", "C")}
    audio_b = [torch.zeros((len(rows), stride), dtype=torch.float32, device="cuda") for rows in of_voice]
    counts = {k: torch.zeros(batch, dtype=torch.int64, device="cuda") for k in audio}
    counts_b = [torch.zeros(len(rows), dtype=torch.int64, device="cuda") for rows in of_voice]
    d_status = torch.zeros(batch, dtype=torch.int32, device="cuda")

    def route_b():
        for v, single in enumerate(singles):
            single.synthesize_targets_device(d_offsets, POOL * 16, d_ids_b[v], d_steps, d_values, None, len(of_voice[v]), STEPS, audio_b[v], stride,
                                             counts_b[v], None, None, stream)

    fns = {
        "A_ms": lambda: plan.synthesize_targets_voices_device(d_offsets, POOL * 16, d_ids, d_steps, d_values, None, d_voices, batch, STEPS, audio["A"],
                                                              stride, counts["A"], None, d_status, stream),
        "B_ms": route_b,
        "C_ms": lambda: singles[0].synthesize_targets_device(d_offsets, POOL * 16, d_ids, d_steps, d_values, None, batch, STEPS, audio["C"], stride,
                                                             counts["C"], None, None, stream),
    }
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    assert int(d_status.abs().sum().item()) == 0
    for v, rows in enumerate(of_voice):
        idx = torch.from_numpy(rows).cuda()
        assert torch.equal(counts["A"][idx], counts_b[v]), v
        assert torch.equal(audio["A"][idx].view(torch.int32), audio_b[v].view(torch.int32)), v
    med, spread = timed_alternating(fns, args.reps, 1)
    results = dict(med, min_max=spread, reps=args.reps, batch=batch, steps_per_utterance=STEPS, voices=names,
                   filter_lengths=[plan.targets_filter_length(v) for v in range(n_voices)], points_per_utterance=points / POOL,
                   samples_per_utterance_by_voice=[plan.targets_voice_output_count(v, STEPS) for v in range(n_voices)], A_equals_B_bytes=True,
                   A_over_B=med["A_ms"] / med["B_ms"], A_over_C=med["A_ms"] / med["C_ms"])
    print(json.dumps(results), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
