"""GPU-box: one stream over a plan of several voices against one single-voice stream per voice (gvtm_stream_create_voices,
DESIGN.md 10).

Five voices x N utterances each (ids interleaved), pushed in pieces of 25 frames (100 ms at 250 Hz) for --rounds rounds:
  mixed       one gvtm_stream_push on a voices stream per round
  sequential  five gvtm_stream_push calls per round, one on a single-voice stream of each voice, one after another
Each push is synchronous (launch, hipDeviceSynchronize, copies); the time of a round is a host clock around the call(s).
Reported: median ms per round of each, and sequential / mixed, for the 0_male voices in float and fp64 (44.1 kHz) and the
5_male voices (model 5, 48 kHz), N = 16 / 52 / 256.
usage: python tests/tools/bench_voices_stream.py [--rounds R] [--piece F] [--per-voice 16,52,256] [--out FILE.json]"""
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
import model5_cases as cases5  # noqa: E402
import tracks  # noqa: E402
from voice_cases import configs, configs5  # noqa: E402
from voice_files import VOICES  # noqa: E402


def model_configs(model):
    if model == "model5":
        return configs5(cases5.RATE)
    return configs(precision=capi.PRECISION_F32 if model == "f32" else capi.PRECISION_F64)


def push_round(stream, block, stride, audio, counts):
    t0 = time.perf_counter()
    stream._plan._check(stream._lib.gvtm_stream_push(stream._h, block.ctypes.data, None, block.shape[1], audio.ctypes.data, stride,
                                                     counts.ctypes.data))
    return time.perf_counter() - t0


def bench(model, per_voice, rounds, piece, warmup):
    cfgs = model_configs(model)
    batch = per_voice * len(VOICES)
    ids = (np.arange(batch) % len(VOICES)).astype(np.int32)
    total = (rounds + warmup) * piece
    base = tracks.random_tracks(16, total, seed0=2024, consonant_heavy=True)
    params = base[np.arange(batch) % 16]
    mixed = g.Stream(g.VoicesPlan(cfgs, 250.0, 0), batch, voice_ids=ids)
    singles = [g.Stream(g.Plan(c, 250.0, 0), per_voice) for c in cfgs]
    sel = [np.nonzero(ids == v)[0] for v in range(len(VOICES))]
    stride = max([mixed.capacity(piece)] + [s.capacity(piece) for s in singles])
    audio = np.zeros((batch, stride), dtype=np.float32)
    counts = np.zeros(batch, dtype=np.int64)
    t_mixed, t_seq = [], []
    for r in range(rounds + warmup):
        block = np.ascontiguousarray(params[:, r * piece: (r + 1) * piece])
        # alternate which form goes first in a round
        order = (0, 1) if r % 2 == 0 else (1, 0)
        for which in order:
            if which == 0:
                t = push_round(mixed, block, stride, audio, counts)
                if r >= warmup:
                    t_mixed.append(t)
            else:
                t = 0.0
                for v, s in enumerate(singles):
                    t += push_round(s, np.ascontiguousarray(block[sel[v]]), stride, audio, counts)
                if r >= warmup:
                    t_seq.append(t)
    row = {"model": model, "per_voice": per_voice, "batch": batch, "piece_frames": piece, "rounds": rounds,
           "mixed_ms_per_round": 1e3 * float(np.median(t_mixed)), "sequential_ms_per_round": 1e3 * float(np.median(t_seq))}
    row["sequential_over_mixed"] = row["sequential_ms_per_round"] / row["mixed_ms_per_round"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--piece", type=int, default=25)
    ap.add_argument("--per-voice", default="16,52,256")
    ap.add_argument("--models", default="f32,f64,model5")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    results = {"voices": VOICES, "piece_frames": args.piece, "rounds": args.rounds, "warmup_rounds": args.warmup,
               "clock": "host perf_counter around each synchronous gvtm_stream_push; median over rounds",
               "compute_units": torch.cuda.get_device_properties(0).multi_processor_count, "rows": []}
    for model in args.models.split(","):
        for per_voice in [int(x) for x in args.per_voice.split(",")]:
            row = bench(model, per_voice, args.rounds, args.piece, args.warmup)
            results["rows"].append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
