"""GPU-box: a ragged batch from event lists in host memory to int16 samples in host memory, three ways.

4096 utterances on the float plan of the male voice (SectionDelay 1, 44.1 kHz), one event list each that yields 50 to 500
frames (fixed seed, about one event per six frames), page-locked buffers, int16 out.  Wall time per synchronous call of
  a  events_packed   gvtm_synthesize_events_packed_host_pcm16: event lists in, packed samples out
  b  packed_frames   gvtm_synthesize_packed_host_pcm16 fed the same utterances' frames, already on the host: the floor,
                     which pays nothing for track generation
  c  device_chain    what a caller that links HIP does without (a): events H2D, gvtm_synthesize_events_chunks_device,
                     gvtm_normalize_batch_device, D2H of the padded int16 rectangle (torch does the copies)
--parent-diag-library FILE: a libgama_vtm_diag.so built at the parent commit; b and c then run on a plan of that library
(the same process, so that the repeats can alternate), else on this build's.  Every variant is warmed up first; the repeats
then alternate the variants.  Per variant: the median, the fastest and the slowest repeat, the bytes it moves each way and
the device time of its synthesis launches (gvtm_plan_set_timing); the tracks kernel's device time on the same lists is
measured on its own (torch events around gvtm_generate_tracks_chunks_device, median), and so is the host's walk over the
lists, which (a) pays before its first copy (gvtm_events_packed_layout alone, median).
usage: python tests/tools/bench_events_packed.py [--reps N] [--batch B] [--parent-diag-library FILE] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, "tests")


def event_lists_for(frame_counts, pool_size=64):
    """One list per utterance that yields exactly frame_counts[b] frames at control period 4: the first n events of a
    pool table (n - 1 about a sixth of the frames), their times spread evenly over the frames, on the grid."""
    import event_lists
    from chunk_cases import starts_plain
    from track_cases import make_singable
    longest = int(max(frame_counts)) // 6 + 2
    pool = [make_singable(event_lists.random_event_table(9000 + k, n_events=longest)) for k in range(pool_size)]
    tables = []
    for b, c in enumerate(frame_counts):
        n = int(c) // 6 + 2
        t = pool[b % pool_size][:n].copy()
        steps = np.linspace(0, int(c), n).round().astype(np.int64)
        steps[-1] = int(c)
        t[:, 0] = 4 * steps
        tables.append(starts_plain(t))
    return tables


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--min-frames", type=int, default=50)
    ap.add_argument("--max-frames", type=int, default=500)
    ap.add_argument("--parent-diag-library", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 5:
        sys.exit("at least five repeats per variant")
    if args.parent_diag_library:
        os.environ["GVTM_DIAG_LIBRARY"] = os.path.abspath(args.parent_diag_library)
    import torch
    import gama_tts_amd as g
    from gama_tts_amd import capi
    from chunk_cases import VARIANT_TRACKS
    from track_cases import product_config
    from voice_cases import configs

    def male(parent):
        plan = g.VoicesPlan(configs(precision=capi.PRECISION_F32, names=["male"]), 250.0, 0, diagnostics=parent)
        plan.set_voice_tracks([product_config(VARIANT_TRACKS[0])])
        return plan

    plan = male(False)
    old = male(True) if args.parent_diag_library else plan
    batch = args.batch
    rng = np.random.default_rng(20240)
    frame_counts = rng.integers(args.min_frames, args.max_frames + 1, size=batch)
    events, chunk_offsets, utt_chunks = plan.pack_event_lists([[t] for t in event_lists_for(frame_counts)])
    fo, offsets = plan.events_packed_layout(events, chunk_offsets, utt_chunks)
    assert np.array_equal(np.diff(fo), frame_counts)
    longest = int(frame_counts.max())
    stride = old.voices_output_capacity(longest)
    pin = dict(events=g.PinnedArray(events.shape, capi.EVENT_DTYPE), out_a=g.PinnedArray((int(offsets[batch]),), np.int16),
               frames=g.PinnedArray((int(fo[batch]), 16), np.float32), out_b=g.PinnedArray((int(offsets[batch]),), np.int16),
               out_c=g.PinnedArray((batch, stride), np.int16))
    pin["events"].array[...] = events
    counts = [np.zeros(batch, np.int64) for _ in range(3)]
    maxabs = [np.zeros(batch, np.float32) for _ in range(2)]
    scales = [np.zeros(batch, np.float32) for _ in range(3)]

    def events_packed(frames_out=None):
        plan.synthesize_events_packed_host_into(pin["events"].array, chunk_offsets, utt_chunks, pin["out_a"].array, None, None, None, frames_out,
                                                counts[0], maxabs[0], scales[0], None)

    events_packed(pin["frames"].array)  # (b)'s input: the frames (a) synthesized
    slices_a = int(plan.packed_stats().slices)

    def packed_frames():
        old.synthesize_packed_host_into(pin["frames"].array, fo, pin["out_b"].array, None, None, counts[1], maxabs[1], scales[1])

    dev = "cuda:0"
    h_events = torch.from_numpy(pin["events"].array.view(np.uint8))
    h_out_c = torch.from_numpy(pin["out_c"].array)
    d_events = torch.empty(h_events.numel() + 296, dtype=torch.uint8, device=dev)
    d_chunk_offsets, d_utt_chunks = torch.from_numpy(chunk_offsets).to(dev), torch.from_numpy(utt_chunks).to(dev)
    d_ids = torch.zeros(batch, dtype=torch.int32, device=dev)
    d_audio = torch.empty((batch, stride), dtype=torch.float32, device=dev)
    d_pcm = torch.empty((batch, stride), dtype=torch.int16, device=dev)
    d_frames, d_counts = torch.empty(batch, dtype=torch.int32, device=dev), torch.empty(batch, dtype=torch.int64, device=dev)
    d_maxabs, d_scales = torch.empty(batch, dtype=torch.float32, device=dev), torch.empty(batch, dtype=torch.float32, device=dev)

    def device_chain():
        stream = torch.cuda.current_stream().cuda_stream
        d_events[: h_events.numel()].copy_(h_events, non_blocking=True)
        old.synthesize_events_chunks_device(d_events, d_chunk_offsets, d_utt_chunks, d_ids, batch, longest, d_audio, stride, d_frames, d_counts, d_maxabs,
                                            None, stream)
        old.normalize_device(d_audio, batch, stride, d_maxabs, d_counts, None, d_pcm, d_scales, stream)
        h_out_c.copy_(d_pcm, non_blocking=True)
        torch.cuda.synchronize()

    fns = {"events_packed": events_packed, "packed_frames": packed_frames, "device_chain": device_chain}
    moved = {"events_packed": {"h2d_bytes": int(events.nbytes + 8 * (chunk_offsets.size + utt_chunks.size) + 16 * (batch + 1)), "d2h_bytes": int(offsets[batch] * 2)},
             "packed_frames": {"h2d_bytes": int(fo[batch] * 64 + 16 * (batch + 1)), "d2h_bytes": int(offsets[batch] * 2)},
             "device_chain": {"h2d_bytes": int(events.nbytes), "d2h_bytes": int(batch * stride * 2)}}
    kernel_ms, slices = {}, {}
    for name, fn in fns.items():  # warm-up, and the device time of each variant's synthesis launches
        p = plan if name == "events_packed" else old
        p.set_timing(True)
        fn()
        p.take_kernel_ms()
        fn()
        ms, launches = p.take_kernel_ms()
        p.set_timing(False)
        kernel_ms[name] = {"synthesis_launches": launches, "synthesis_ms_sum": ms * launches}
        slices[name] = int(p.packed_stats().slices) if name != "device_chain" else 1
    staging = int(plan.packed_stats().staging_bytes)
    # the three agree, utterance by utterance
    c_counts, c_scales = d_counts.cpu().numpy(), d_scales.cpu().numpy()
    same = np.array_equal(counts[0], counts[1]) and np.array_equal(counts[0], c_counts) and np.array_equal(scales[0], scales[1]) and np.array_equal(scales[0], c_scales)
    same = same and np.array_equal(pin["out_a"].array, pin["out_b"].array)
    for b in range(batch):
        n = int(counts[0][b])
        same = same and np.array_equal(pin["out_a"].array[offsets[b]: offsets[b] + n], pin["out_c"].array[b, :n])
    # the tracks kernel alone on the same lists, device resident
    d_rows = torch.empty((batch, longest, 16), dtype=torch.float32, device=dev)
    tracks_ms = []
    for _ in range(21):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        plan.generate_tracks_chunks_device(d_events, d_chunk_offsets, d_utt_chunks, d_ids, batch, longest, d_rows, d_frames, None, torch.cuda.current_stream().cuda_stream)
        stop.record()
        torch.cuda.synchronize()
        tracks_ms.append(start.elapsed_time(stop))
    tracks = float(np.median(tracks_ms[1:]))
    # and on one slice of it (the walk is a chain of dependent steps: as long as the longest list, however few the lists)
    per_slice = int(plan.packed_stats().largest_slice)
    slice_ms = []
    for _ in range(21):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        plan.generate_tracks_chunks_device(d_events, d_chunk_offsets, d_utt_chunks, d_ids, per_slice, longest, d_rows, d_frames, None, torch.cuda.current_stream().cuda_stream)
        stop.record()
        torch.cuda.synchronize()
        slice_ms.append(start.elapsed_time(stop))
    tracks_slice = float(np.median(slice_ms[1:]))

    # the host's walk over the lists, which (a) pays in front of its first copy: the layout call alone
    layout_ms = []
    for _ in range(9):
        t0 = time.perf_counter()
        plan.events_packed_layout(pin["events"].array, chunk_offsets, utt_chunks)
        layout_ms.append((time.perf_counter() - t0) * 1e3)
    layout = float(np.median(layout_ms))

    times = {name: [] for name in fns}
    for _ in range(args.reps):
        for name, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
    result = {"batch": batch, "frames": [args.min_frames, args.max_frames], "mean_frames": float(frame_counts.mean()), "events": int(events.shape[0]),
              "reps": args.reps, "output": "int16", "precision": "float", "b_and_c_library": "parent commit" if args.parent_diag_library else "this build",
              "identical_samples_counts_scales": bool(same), "events_packed_staging_bytes": staging, "events_packed_slices_with_frames_out": slices_a,
              "tracks_kernel_ms": tracks, "tracks_kernel_ms_one_slice": tracks_slice, "largest_slice": per_slice, "host_layout_ms": layout, "variants": {}}
    for name in fns:
        t = np.array(times[name])
        row = {"ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max()), "spread": float((t.max() - t.min()) / np.median(t)), "slices": slices[name]}
        row.update(moved[name])
        row.update(kernel_ms[name])
        result["variants"][name] = row
    v = result["variants"]
    result["a_beats_c"] = bool(v["events_packed"]["ms"] < v["device_chain"]["ms"])
    result["a_within_b_bracket_plus_tracks"] = bool(v["events_packed"]["ms"] <= v["packed_frames"]["max_ms"] + tracks)
    print(json.dumps(result), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    for p in pin.values():
        p.close()


if __name__ == "__main__":
    main()
