"""Host arrays on and off the device for the GPU tests: inputs as tensors on cuda:0, outputs that start out zero or filled
with a pattern (how a test sees that nothing was written where nothing should be), one call on the current stream,
synchronize, numpy back.  torch is imported inside the functions: collecting the tests needs no GPU."""
import collections

import numpy as np

from gama_tts_amd import capi

EventsOut = collections.namedtuple("EventsOut", "audio frames counts maxabs drift")


def to_device(*arrays):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in arrays)


def filled(shape, value, dtype):
    """A tensor of numpy type `dtype` on cuda:0, every element `value`."""
    import torch
    return torch.full(shape if isinstance(shape, tuple) else (shape,), value, dtype=getattr(torch, np.dtype(dtype).name), device="cuda:0")


def current_stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def to_host(*tensors):
    import torch
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in tensors)


def events_on_device(tables):
    """Event tables -> (the records back to back as bytes, int64 offsets [B + 1]) on the device."""
    evs = [capi.events_from_table(t) for t in tables]
    offsets = np.zeros(len(evs) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(e) for e in evs])
    return to_device(np.concatenate(evs).view(np.uint8), offsets)


def run_batch_device(plan, params, frames, stride):
    """gvtm_synthesize_batch_device with device-resident frame counts -> (audio [B][stride], counts); no peaks asked for."""
    batch, max_frames = params.shape[:2]
    dp, df = to_device(params, frames)
    da, dc = filled((batch, stride), 0.0, np.float32), filled(batch, 0, np.int64)
    plan.synthesize_device(dp, batch, max_frames, da, stride, df, dc, None, current_stream())
    return to_host(da, dc)


def run_voices_device(plan, params, ids, frames, stride, fill=0.0):
    """gvtm_synthesize_voices_device -> (audio [B][stride] that started out as `fill`, counts, maxabs that started out 5.0)."""
    batch, max_frames = params.shape[:2]
    dp, di, df = to_device(params, ids, frames)
    da, dc, dm = filled((batch, stride), fill, np.float32), filled(batch, 0, np.int64), filled(batch, 5.0, np.float32)
    plan.synthesize_voices_device(dp, di, batch, max_frames, da, stride, df, dc, dm, current_stream())
    return to_host(da, dc, dm)


def generate_tracks(tables, max_frames, drift0, track_config=None, plan=None, ids=None):
    """gvtm_generate_tracks_device under track_config, or (plan and ids given) gvtm_generate_tracks_voices_device ->
    (frames [B][max_frames][16], counts, drift states after).  The voices entry's frames start out 7.0 and its counts 99;
    the single-configuration kernel's start out zero."""
    batch = len(tables)
    d_events, d_offsets = events_on_device(tables)
    d_drift, = to_device(drift0.copy())
    if ids is None:
        d_params, d_counts = filled((batch, max_frames, 16), 0.0, np.float32), filled(batch, 0, np.int32)
        capi.generate_tracks_device(track_config, d_events, d_offsets, batch, max_frames, d_params, d_counts, d_drift, current_stream())
    else:
        d_ids, = to_device(np.asarray(ids, dtype=np.int32))
        d_params, d_counts = filled((batch, max_frames, 16), 7.0, np.float32), filled(batch, 99, np.int32)
        plan.generate_tracks_voices_device(d_events, d_offsets, d_ids, batch, max_frames, d_params, d_counts, d_drift, current_stream())
    return to_host(d_params, d_counts, d_drift)


def synthesize_events(plan, tables, max_frames, stride, drift0, ids=None, track_config=None, fill=0.0):
    """gvtm_synthesize_events_voices_device (ids given) or gvtm_synthesize_events_device (track_config given) ->
    dict of audio [B][stride], frames int32 [B], counts int64 [B], maxabs [B], drift [B][5]; the audio starts out as
    `fill`, frames and counts 99, maxabs 5.0."""
    batch = len(tables)
    d_events, d_offsets = events_on_device(tables)
    out = dict(audio=filled((batch, stride), fill, np.float32), frames=filled(batch, 99, np.int32), counts=filled(batch, 99, np.int64),
               maxabs=filled(batch, 5.0, np.float32), drift=to_device(drift0.copy())[0])
    if ids is not None:
        d_ids, = to_device(np.asarray(ids, dtype=np.int32))
        plan.synthesize_events_voices_device(d_events, d_offsets, d_ids, batch, max_frames, out["audio"], stride, out["frames"],
                                             out["counts"], out["maxabs"], out["drift"], current_stream())
    else:
        plan.synthesize_events_device(track_config, d_events, d_offsets, batch, max_frames, out["audio"], stride, out["frames"],
                                      out["counts"], out["maxabs"], out["drift"], current_stream())
    return dict(zip(out, to_host(*out.values())))


def events_to_audio(plan, track_config, tables, max_frames):
    """gvtm_generate_tracks_device then gvtm_synthesize_batch_device, the frames produced and consumed in device memory ->
    (audio [B][output_count(max_frames)], frame counts, sample counts)."""
    batch = len(tables)
    d_events, d_offsets = events_on_device(tables)
    d_params, d_frames = filled((batch, max_frames, 16), 0.0, np.float32), filled(batch, 0, np.int32)
    capi.generate_tracks_device(track_config, d_events, d_offsets, batch, max_frames, d_params, d_frames, None, current_stream())
    stride = plan.output_count(max_frames)
    d_audio, d_counts = filled((batch, stride), 0.0, np.float32), filled(batch, 0, np.int64)
    plan.synthesize_device(d_params, batch, max_frames, d_audio, stride, d_frames, d_counts, None, current_stream())
    return to_host(d_audio, d_frames, d_counts)


def events_chain_and_entry(plan, track_config, tables, max_frames, stride, drift0, maxabs=True):
    """The two-call chain (gvtm_generate_tracks_device, then gvtm_synthesize_batch_device on its frames) and
    gvtm_synthesize_events_device on the same lists, each with zeroed outputs and a copy of drift0 of its own ->
    (chain, entry, the chain's frames): chain and entry an EventsOut each (maxabs None if not asked for).  Unlike the other
    helpers' results these stay on the device, synchronized: the callers compare whole batches there, bit for bit."""
    import torch
    batch = len(tables)
    d_events, d_offsets = events_on_device(tables)

    def fresh():
        return EventsOut(filled((batch, stride), 0.0, np.float32), filled(batch, 0, np.int32), filled(batch, 0, np.int64),
                         filled(batch, 0.0, np.float32) if maxabs else None, to_device(drift0.copy())[0])

    chain, entry = fresh(), fresh()
    d_params = filled((batch, max_frames, 16), 0.0, np.float32)
    capi.generate_tracks_device(track_config, d_events, d_offsets, batch, max_frames, d_params, chain.frames, chain.drift, current_stream())
    plan.synthesize_device(d_params, batch, max_frames, chain.audio, stride, chain.frames, chain.counts, chain.maxabs, current_stream())
    plan.synthesize_events_device(track_config, d_events, d_offsets, batch, max_frames, entry.audio, stride, entry.frames,
                                  entry.counts, entry.maxabs, entry.drift, current_stream())
    torch.cuda.synchronize()
    return chain, entry, d_params
