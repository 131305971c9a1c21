"""GPU-box: utterances of several event lists (gvtm_generate_tracks_chunks_device).

What the per-chunk restart (table rebuild, first deltas, staged boundary) costs: 4096 utterances x 4 chunks x 20 events
through the chunks kernel beside bench_tracks.py's 4096 x 80 events through the voices kernel and, for the kernel's own
overhead, the same 80-event lists as one-chunk utterances through the chunks kernel.  Five voices interleaved, everything
resident, one process; the variants alternate inside every repeat after warm-up launches; medians, time between HIP events.
A measurement, not a gate.
usage: python tests/tools/bench_tracks_chunks.py [--reps N] [--out FILE.json]"""
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
import event_lists  # noqa: E402
from bench_tracks_voices import timed_alternating  # noqa: E402
from chunk_cases import chunks_on_device, offset_tables  # noqa: E402
from device_io import events_on_device  # noqa: E402
from voice_cases import configs, track_configs  # noqa: E402
from voice_files import VOICES  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    batch = args.batch
    stream = torch.cuda.current_stream().cuda_stream
    tcs = track_configs()
    plan = g.VoicesPlan(configs(precision=capi.PRECISION_F32), 250.0, 0)
    plan.set_voice_tracks(tcs)

    long_tables = [event_lists.random_event_table(s, n_events=80, control_period=4, max_gap_periods=12) for s in range(64)]
    short_tables = [event_lists.random_event_table(1000 + s, n_events=20, control_period=4, max_gap_periods=12) for s in range(256)]
    whole = [long_tables[b % 64] for b in range(batch)]
    chunked = [[short_tables[(4 * b + c) % 256] for c in range(4)] for b in range(batch)]
    max_frames = max([capi.tracks_frame_count(tcs[0], capi.events_from_table(t)) for t in long_tables]
                     + [capi.tracks_chunks_frame_count(tcs[0], *offset_tables([u])[:2]) for u in chunked[:64]])
    d_events, d_offsets = events_on_device(whole)
    d_one = torch.arange(batch + 1, dtype=torch.int64, device="cuda")  # one chunk per utterance: d_offsets are the chunk offsets
    c_events, c_chunk_offsets, c_utt_chunks = chunks_on_device(chunked)
    d_ids = torch.from_numpy((np.arange(batch) % len(VOICES)).astype(np.int32)).cuda()
    d_params = torch.zeros((batch, max_frames, 16), dtype=torch.float32, device="cuda")
    counts = {k: torch.zeros(batch, dtype=torch.int32, device="cuda") for k in ("voices", "one", "four")}
    med, spread = timed_alternating({
        "voices_80_events_ms": lambda: plan.generate_tracks_voices_device(d_events, d_offsets, d_ids, batch, max_frames, d_params, counts["voices"], None, stream),
        "chunks_1x80_events_ms": lambda: plan.generate_tracks_chunks_device(d_events, d_offsets, d_one, d_ids, batch, max_frames, d_params, counts["one"], None, stream),
        "chunks_4x20_events_ms": lambda: plan.generate_tracks_chunks_device(c_events, c_chunk_offsets, c_utt_chunks, d_ids, batch, max_frames, d_params, counts["four"], None, stream),
    }, args.reps, 20)
    assert torch.equal(counts["voices"], counts["one"])
    results = dict(med, batch=batch, reps=args.reps, min_max=spread, frames_total_80=int(counts["voices"].sum().item()),
                   frames_total_4x20=int(counts["four"].sum().item()))
    print(json.dumps(results), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
