"""GPU-box: a session that listens (gvtm_stream_listen) beside the route that exists without it and beside a
session that does not listen at all, on the same utterances.

Float plan of the male voice, SectionDelay 1, 4096 utterances in lockstep (a pool of 16 distinct ones tiled over the batch),
targets-fed pushes of 1200 steps until two rings of 65 536 samples have completed; Blackman window, log scale, all bins.
  listening  audio NULL, gvtm_stream_take_spectra after every push that completes a ring
  today      the parent's route to the same spectra: audio to the host on every push, the rings assembled on the host, uploaded
             when full, gvtm_analyze_spectrum_device, the spectra downloaded
  plain      no listener, audio to the host: what a session costs without any spectrum (the price of listening itself is
             listening against this)
Wall clock around each push with everything its route does behind it (the tables of every push are packed beforehand), the
routes alternating inside every repeat; mean and spread of the repeats after one warm-up session each, whose spectra
(listening, today) and sample counts (all) are compared.  --routes plain with GVTM_LIBRARY naming another build gives the
plain session of that build.
usage: python tests/tools/stream_listen_ab.py [--reps N] [--batch B] [--routes a,b] [--out FILE.json]"""
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
from stream_targets_ab import tiled_tables  # noqa: E402
from voice_cases import male_plan  # noqa: E402

POOL, STEPS, RING, RINGS = 16, 1200, 65536, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--routes", default="listening,today,plain")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    batch, routes = args.batch, args.routes.split(",")
    plan = male_plan(precision=capi.PRECISION_F32)
    lib, p = plan._lib, capi._ptr
    # the pushes: as many as bring two rings' worth of samples (a push of a multiple of 12 steps synthesizes all of them; the
    # count asked here includes what only a finish flushes, hence the margin)
    pushes = 1
    while plan.targets_output_count(pushes * STEPS) < RINGS * RING + 600:
        pushes += 1
    total = pushes * STEPS
    pool = [cases.spoken_lists(total, seed) for seed in range(POOL)]
    tables = [tiled_tables([sessions.slice_lists(u, i * STEPS, STEPS) for u in pool], batch) for i in range(pushes)]
    stream = g.Stream(plan, batch)
    stride = stream.targets_capacity(STEPS)
    audio, counts = np.zeros((batch, stride), np.float32), np.zeros(batch, np.int64)
    an = g.Analysis(capi.WINDOW_BLACKMAN, RING, True, -120.0, 0.0, 44100, device=0) if routes != ["plain"] else None
    n_bins = an.n_bins if an else 0
    spectra = np.zeros((batch, 1, n_bins), np.float32) if an else None
    host_rings = np.zeros((batch, RING), np.float32) if "today" in routes else None
    ring_counts = torch.full((batch,), RING, dtype=torch.int64, device="cuda:0")

    def run(route, keep=None):
        """One session -> (seconds per push, which pushes completed a ring); keep: takes (per push the counts, per ring the
        spectra of the pool's utterances)."""
        plan._check(lib.gvtm_stream_reset(stream._h))
        if route == "listening":
            stream.listen(an, 1, spectra=True, signal=False)
        times, completing, fill = [], [], 0
        for i in range(pushes):
            offsets, steps, values = tables[i]
            t0 = time.perf_counter()
            out = None if route == "listening" else audio
            plan._check(lib.gvtm_stream_push_targets(stream._h, p(offsets), p(steps), p(values), None, STEPS, p(out), stride, p(counts), None))
            n = int(counts[0])  # (lockstep)
            done = (fill + n) // RING
            if route == "listening" and done:
                plan._check(lib.gvtm_stream_take_spectra(stream._h, p(spectra), None, None))
            elif route == "today":
                head = min(n, RING - fill)
                host_rings[:, fill: fill + head] = audio[:, :head]
                if done:
                    d_rings = torch.from_numpy(host_rings).to("cuda:0")
                    d_spectra = torch.empty((batch, 1, n_bins), dtype=torch.float32, device="cuda:0")
                    an.analyze_device(d_rings, RING, ring_counts, batch, 1, None, d_spectra, None, None, torch.cuda.current_stream().cuda_stream)
                    spectra[:] = d_spectra.cpu().numpy()
                    host_rings[:, : n - head] = audio[:, head: n]
            times.append(time.perf_counter() - t0)
            assert done <= 1
            completing.append(bool(done))
            fill = (fill + n) % RING
            if keep is not None:
                keep.append((n, spectra[:POOL, 0].copy() if done and route != "plain" else None))
        if route == "listening":
            stream.unlisten()
        return times, completing

    kept = {route: [] for route in routes}
    for route in routes:
        assert sum(run(route, kept[route])[1]) == RINGS
    for route in routes[1:]:
        assert [n for n, _ in kept[route]] == [n for n, _ in kept[routes[0]]]
    same_spectra = None
    if "listening" in routes and "today" in routes:
        rings = [(a, b) for (_, a), (_, b) in zip(kept["listening"], kept["today"]) if a is not None]
        assert len(rings) == RINGS and all(b is not None for _, b in rings)
        same_spectra = all(a.tobytes() == b.tobytes() for a, b in rings)
        assert same_spectra

    runs = {route: [] for route in routes}
    for _ in range(args.reps):
        for route in routes:
            runs[route].append(run(route))
    per_push_samples = [n for n, _ in kept[routes[0]]]
    result = dict(batch=batch, pushes=pushes, steps_per_push=STEPS, reps=args.reps, rings=RINGS, n_bins=n_bins, samples_per_push=per_push_samples[1],
                  audio_stride=stride, same_spectra=same_spectra, library=os.environ.get("GVTM_LIBRARY", "this tree"))
    for route, sessions_run in runs.items():
        sums = [sum(t) for t, _ in sessions_run]
        per_push = np.mean(np.asarray([t for t, _ in sessions_run]), axis=0)
        completing = np.asarray(sessions_run[0][1])
        result[route + "_session_ms"] = 1e3 * float(np.mean(sums))
        result[route + "_session_min_max_ms"] = [1e3 * min(sums), 1e3 * max(sums)]
        result[route + "_push_ms_not_completing"] = 1e3 * float(per_push[~completing].mean())
        result[route + "_push_ms_completing"] = 1e3 * float(per_push[completing].mean())
    # bytes per push, beside the targets' tables every route uploads: host to device / device to host, (a push that completes
    # no ring, one that does)
    table, count_bytes, audio_bytes, spectra_bytes, ring_bytes = batch * (8 * 8 + 2 * 4), 8 * batch, 4 * batch * stride, 4 * batch * n_bins, 4 * batch * RING
    result["bytes_per_push"] = {
        "listening": {"h2d": [table, table], "d2h": [count_bytes, count_bytes + spectra_bytes]},
        "today": {"h2d": [0, ring_bytes], "d2h": [count_bytes + audio_bytes, count_bytes + audio_bytes + spectra_bytes]},
        "plain": {"h2d": [0, 0], "d2h": [count_bytes + audio_bytes, count_bytes + audio_bytes]}}
    print(json.dumps(result), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
