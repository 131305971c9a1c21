"""GPU-box: event lists from posture sequences on the device (gvtm_generate_events_device,
gvtm_synthesize_postures_device).

4096 utterances of the 54-posture sentence of tests/golden/rules_golden.npz (288 events each), float plan of the male voice,
control period 4 ms:
  generate    one gvtm_generate_events_device call (count, scan, write), with the bytes it writes
  parent      the ready-made events copied from page-locked memory, then gvtm_synthesize_events_device: what a caller did
              before, once it had the lists (making them, generateEventList() per utterance on a host core, is outside)
  postures    the postures copied from page-locked memory, then gvtm_synthesize_postures_device
Before anything is timed the device's lists are compared with gvtm_rules_apply_host's, byte for byte, and the two routes'
samples with each other.  The variants of a comparison alternate inside every repeat; medians, wall time between HIP events.
With --kernels the script only calls gvtm_generate_events_device twenty times, for a kernel trace taken around it.
usage: python tests/tools/bench_rules.py [--reps N] [--batch B] [--kernels] [--out FILE.json]"""
import argparse
import json
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
sys.path.insert(0, "tests/tools")
import gama_tts_amd as g  # noqa: E402
from gama_tts_amd import capi  # noqa: E402
import oracle  # noqa: E402
import rules_cases as cases  # noqa: E402
from bench_tracks_voices import timed_alternating  # noqa: E402

ENTRY = "sentence.0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    batch = args.batch
    stream = torch.cuda.current_stream().cuda_stream
    golden = np.load(cases.GOLDEN)
    rules = capi.Rules(cases.model_arrays(golden, "0_male"), device=0)
    one = capi.postures_from_table(cases.posture_records(golden, ENTRY))
    events, _, _, status = rules.apply_host(4, one)
    assert status == 0
    n_postures, n_events = len(one), len(events)
    postures = np.tile(one, batch)
    offsets = (np.arange(batch + 1, dtype=np.int64) * n_postures)
    event_offsets = (np.arange(batch + 1, dtype=np.int64) * n_events)
    capacity = batch * n_events
    results = {"batch": batch, "postures": n_postures, "events": n_events, "reps": args.reps,
               "posture_bytes": int(postures.nbytes), "event_bytes": int(capacity * capi.EVENT_DTYPE.itemsize)}

    d_postures = torch.from_numpy(postures.view(np.uint8)).cuda()
    d_offsets = torch.from_numpy(offsets).cuda()
    d_events = torch.empty(capacity * capi.EVENT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_event_offsets = torch.empty(batch + 1, dtype=torch.int64, device="cuda")
    d_status = torch.empty(batch, dtype=torch.int32, device="cuda")

    def generate():
        rules.generate_events_device(4, d_postures, d_offsets, batch, d_events, capacity, d_event_offsets, d_status=d_status, stream=stream)

    if args.kernels:
        for _ in range(20):
            generate()
        torch.cuda.synchronize()
        return
    generate()
    torch.cuda.synchronize()
    got = d_events.cpu().numpy().reshape(batch, -1)
    assert (d_status.cpu().numpy() == 0).all() and np.array_equal(d_event_offsets.cpu().numpy(), event_offsets)
    assert (got == events.view(np.uint8)[None, :]).all(), "the device's lists differ from the host rule's"
    med, span = timed_alternating({"generate": generate}, args.reps, 20)
    results["generate_ms"], results["generate_span"] = med["generate"], span["generate"]
    results["generate_GBps_written"] = results["event_bytes"] / med["generate"] / 1e6

    # --- the two routes to samples
    plan = g.Plan(g.config_from_dict(g.read_config_file(oracle.VOICE_MALE), 44100.0, 1, capi.PRECISION_F32), 250.0, 0)
    config = capi.TrackConfig(control_period_ms=4, macro_intonation=0, micro_intonation=1, intonation_drift=1, smooth_intonation=1,
                              initial_pitch=0.0, mean_pitch=-12.0, drift_deviation=1.0, drift_sample_rate=250.0, drift_lowpass_cutoff=4.0)
    max_frames = capi.tracks_frame_count(config, events)
    stride = plan.output_count(max_frames)
    results["frames"], results["samples"] = int(max_frames), int(stride)
    host_events = torch.from_numpy(np.tile(events, batch).view(np.uint8)).pin_memory()
    host_event_offsets = torch.from_numpy(event_offsets).pin_memory()
    host_postures = torch.from_numpy(postures.view(np.uint8)).pin_memory()
    host_offsets = torch.from_numpy(offsets).pin_memory()
    d_in_events = torch.empty_like(d_events)
    d_in_offsets = torch.empty_like(d_event_offsets)
    audio = [torch.zeros((batch, stride), dtype=torch.float32, device="cuda") for _ in range(2)]
    counts = [torch.zeros(batch, dtype=torch.int64, device="cuda") for _ in range(2)]
    peaks = [torch.zeros(batch, dtype=torch.float32, device="cuda") for _ in range(2)]

    def parent():
        d_in_events.copy_(host_events, non_blocking=True)
        d_in_offsets.copy_(host_event_offsets, non_blocking=True)
        plan.synthesize_events_device(config, d_in_events, d_in_offsets, batch, max_frames, audio[0], stride, None, counts[0], peaks[0], None, stream)

    def from_postures():
        d_postures.copy_(host_postures, non_blocking=True)
        d_offsets.copy_(host_offsets, non_blocking=True)
        plan.synthesize_postures_device(rules, config, d_postures, d_offsets, capacity, batch, max_frames, audio[1], stride, None, counts[1], peaks[1], None,
                                        d_status, stream)

    def upload_events():
        d_in_events.copy_(host_events, non_blocking=True)
        d_in_offsets.copy_(host_event_offsets, non_blocking=True)

    def upload_postures():
        d_postures.copy_(host_postures, non_blocking=True)
        d_offsets.copy_(host_offsets, non_blocking=True)

    parent()
    from_postures()
    torch.cuda.synchronize()
    assert torch.equal(counts[0], counts[1]) and torch.equal(peaks[0], peaks[1]) and torch.equal(audio[0], audio[1]), "the two routes' samples differ"
    results["samples_compared"] = int(counts[0].sum().item())
    med, span = timed_alternating({"parent": parent, "postures": from_postures, "upload_events": upload_events, "upload_postures": upload_postures},
                                  args.reps, 1)
    for k in med:
        results[k + "_ms"], results[k + "_span"] = med[k], span[k]
    print(json.dumps(results))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
