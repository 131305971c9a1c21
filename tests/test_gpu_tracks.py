"""Track generation on the device (gvtm_generate_tracks_*) against the reference fixtures and the oracle:
bit-identical frames, frame counts and drift-generator states; and events -> frames -> audio with the frames
never leaving the device."""
import numpy as np
import pytest

from gama_tts_amd import capi
import event_lists
import oracle
from device_io import events_chain_and_entry, events_on_device, events_to_audio
from parity_rules import TOL, check_model5, peak_err, within, largest_error_within
from track_cases import fresh_drift, product_config, singable_event_table, used_drift
from voice_cases import male5_plan, male_plan

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", event_lists.CAPTURED)
def test_device_matches_captured_reference_calls(name, golden_tracks):
    state = [oracle.FRESH_DRIFT]
    for call in range(6):
        cfg, events, frames = event_lists.load_golden(golden_tracks, name, call)
        params, counts, drift = capi.generate_tracks_host(product_config(cfg), [capi.events_from_table(events)], frames.shape[0] + 3, drift=state)
        assert counts[0] == frames.shape[0]
        assert np.array_equal(params[0, : frames.shape[0]].view(np.uint32), frames.view(np.uint32)), (name, call)
        assert not params[0, frames.shape[0]:].any()
        state = [tuple(drift[0])]
        _, want_state = oracle.tracks_generate(oracle.track_config(cfg), events, oracle.FRESH_DRIFT) if call == 0 else (None, None)
        if call == 0:
            assert state[0] == want_state


@pytest.mark.parametrize("flags", [(1, 1, 1, 1), (0, 1, 0, 1), (1, 0, 1, 0), (0, 0, 0, 0)])
def test_ragged_batch_against_oracle(flags):
    macro, micro, drift, smooth = flags
    cfg = np.array([4, macro, micro, drift, smooth, -20.0, -6.0, 4.0, 250.0, 4.0])
    # (lists of up to 240 events get the kernel's table in LDS; 260 walks device memory; test_gpu_tracks_edges.py crosses the line)
    tables = [event_lists.random_event_table(100 + b, n_events=int(n)) for b, n in enumerate([40, 2, 1, 17, 80, 3, 55, 9, 33, 110, 111, 150, 260])]
    want = [oracle.tracks_generate(oracle.track_config(cfg), t) for t in tables]
    max_frames = max(w[0].shape[0] for w in want)
    params, counts, dr = capi.generate_tracks_host(product_config(cfg), [capi.events_from_table(t) for t in tables], max_frames,
                                                   drift=[oracle.FRESH_DRIFT] * len(tables))
    for b, (frames, state) in enumerate(want):
        assert counts[b] == frames.shape[0]
        assert np.array_equal(params[b, : frames.shape[0]].view(np.uint32), frames.view(np.uint32)), b
        assert tuple(dr[b]) == state


def test_truncation_and_fresh_generator_default():
    cfg = np.array([4, 1, 1, 1, 1, -20.0, -6.0, 4.0, 250.0, 4.0])
    table = event_lists.random_event_table(7, n_events=30)
    frames, _ = oracle.tracks_generate(oracle.track_config(cfg), table)
    params, counts, _ = capi.generate_tracks_host(product_config(cfg), [capi.events_from_table(table)], 50)  # drift=None: fresh generator
    assert counts[0] == frames.shape[0] > 50
    assert np.array_equal(params[0].view(np.uint32), frames[:50].view(np.uint32))


def test_host_entry_with_an_empty_event_array():
    """Three utterances without an event: no frame, the rows zero, the generators where they were -- as the host's count and
    the oracle say."""
    cfg = np.array([4, 1, 1, 1, 1, -20.0, -6.0, 4.0, 250.0, 4.0])
    tables = [event_lists.random_event_table(60 + b, n_events=0) for b in range(3)]
    lists = [capi.events_from_table(t) for t in tables]
    drift0 = used_drift(3)
    params, counts, dr = capi.generate_tracks_host(product_config(cfg), lists, 4, drift=[tuple(d) for d in drift0])
    assert counts.tolist() == [capi.tracks_chunks_frame_count(product_config(cfg), e, np.zeros(2, np.int64)) for e in lists] == [0, 0, 0]
    assert not params.any() and params.shape == (3, 4, 16)
    for b, t in enumerate(tables):  # (the device entry refuses a null events pointer, which is what no event at all gives it)
        frames, state = oracle.tracks_generate(oracle.track_config(cfg), t, tuple(drift0[b]))
        assert frames.shape[0] == 0 and tuple(dr[b]) == state == tuple(drift0[b])
    # no frames asked for either: nothing comes back but the counts
    params0, counts0, _ = capi.generate_tracks_host(product_config(cfg), lists, 0)
    assert params0.shape == (3, 0, 16) and not counts0.any()


def test_events_to_audio_on_the_device(golden_tracks):
    """Event lists -> parameter frames -> audio, the frames produced and consumed in device memory: equals the
    oracle of the oracle (EventList::generateOutput then the vocal-tract model)."""
    names = ["hello", "question", "count", "hello"]
    cfgv, _, _ = event_lists.load_golden(golden_tracks, "hello", 0)
    tables = [event_lists.load_golden(golden_tracks, n, 0)[1] for n in names]
    want_frames = [oracle.tracks_generate(oracle.track_config(cfgv), t)[0] for t in tables]
    max_frames = max(f.shape[0] for f in want_frames)
    audio, frame_counts, counts = events_to_audio(male_plan(), product_config(cfgv), tables, max_frames)
    cfg = oracle.male_config()
    for b, frames in enumerate(want_frames):
        assert frame_counts[b] == frames.shape[0]
        ref = oracle.synthesize(cfg, frames)
        assert counts[b] == ref.size
        assert within(audio[b, : ref.size], ref, 1e-9), (b, peak_err(audio[b, : ref.size], ref))


def test_events_to_audio_on_the_device_model5(golden_tracks):
    """The same chain into reference model 5 (the event list and its frames do not depend on the vocal-tract model):
    frames made on the device feed the model-5 kernel without leaving HBM."""
    names = ["question", "hello", "count"]
    cfgv, _, _ = event_lists.load_golden(golden_tracks, "hello", 0)
    tables = [event_lists.load_golden(golden_tracks, n, 0)[1] for n in names]
    want_frames = [oracle.tracks_generate(oracle.track_config(cfgv), t)[0] for t in tables]
    max_frames = max(f.shape[0] for f in want_frames)
    audio, _, counts = events_to_audio(male5_plan(), product_config(cfgv), tables, max_frames)
    cfg = oracle.male5_config(48000.0)
    for b, frames in enumerate(want_frames):
        ref, _ = oracle.synthesize5(cfg, frames)
        assert counts[b] == ref.size
        check_model5(audio[b, : ref.size], ref)


@pytest.mark.parametrize("batch", [5, 300, 601], ids=["one_row", "two_rows", "four_rows"])
@pytest.mark.parametrize("precision", [capi.PRECISION_F32, capi.PRECISION_F64, capi.PRECISION_MIXED], ids=["f32", "f64", "mixed"])
@pytest.mark.parametrize("delay", [1, 2], ids=["d1", "d2"])
def test_events_entry_equals_the_two_call_chain(batch, precision, delay):
    """gvtm_synthesize_events_device (event lists in, samples out, the frames in a buffer the plan owns): samples, sample
    counts, frame counts, peaks and drift-generator states must be those of gvtm_generate_tracks_device followed by
    gvtm_synthesize_batch_device, bit for bit, in every workgroup shape the product picks; one utterance is also taken
    through the oracle of the oracle (frames by the tracks oracle, pinned to captured generateOutput() calls, then the
    vocal-tract oracle)."""
    import torch
    if batch > 5 and delay == 2 and precision == capi.PRECISION_MIXED:
        pytest.skip("covered by the other combinations")
    cfgv = np.array([4, 1, 1, 1, 1, -20.0, -6.0, 4.0, 250.0, 4.0])
    pool_n = [40, 2, 1, 17, 60, 3, 55, 9, 33, 25, 48]
    pool = [singable_event_table(300 + b, n) for b, n in enumerate(pool_n)]
    tables = [pool[b % len(pool)] for b in range(batch)]
    tc = product_config(cfgv)
    frames_of = [capi.tracks_frame_count(tc, capi.events_from_table(t)) for t in pool]
    max_frames = max(frames_of)
    plan = male_plan(delay=delay, precision=precision)
    stride = plan.output_capacity(max_frames)
    # generators that have run before; the two-call chain (frames in device memory) and the one call
    chain, entry, d_params = events_chain_and_entry(plan, tc, tables, max_frames, stride, used_drift(batch))
    a1, f1, n1, m1, dr1 = chain
    a2, f2, n2, m2, dr2 = entry
    # (random event lists can still hold combinations the model itself cannot sing -- a parameter plus its "special" offset
    # outside its range -- and an utterance that goes non-finite says nothing: compared are the ones that stay finite)
    ok = torch.isfinite(a1).all(dim=1) & torch.isfinite(m1)
    assert int(ok[:len(pool)].sum().item()) >= (len(pool) * 2) // 3 or batch <= 5
    assert torch.equal(f1, f2) and torch.equal(n1, n2)
    assert torch.equal(dr1.view(torch.int64), dr2.view(torch.int64))
    assert torch.equal(m1[ok].view(torch.int32), m2[ok].view(torch.int32))
    assert torch.equal(a1[ok].view(torch.int32), a2[ok].view(torch.int32))
    assert f2[:len(pool)].cpu().tolist() == frames_of[:batch]
    # utterance 0 against the oracles (through the chain's own frames, which carry its drift generator's history)
    frames4 = d_params[0, : frames_of[0]].cpu().numpy()
    ref = oracle.synthesize(oracle.male_config(44100.0, delay, float_model=int(precision == capi.PRECISION_F32)), frames4)
    got = a2[0, : ref.size].cpu().numpy()
    assert n2[0].item() == ref.size and np.isfinite(ref).all()
    if precision == capi.PRECISION_F32:
        assert np.array_equal(got, ref)
    else:
        assert largest_error_within(got, ref, TOL[precision])


def test_events_entry_truncates_at_max_frames_and_serves_every_model():
    """A list that yields more frames than the rows hold is cut at max_frames (frame count still reported in full, drift state
    that of the whole list); SectionDelay 3 and reference model 5 take the same call."""
    import torch
    cfgv = np.array([4, 1, 1, 1, 1, -20.0, -6.0, 4.0, 250.0, 4.0])
    tc = product_config(cfgv)
    tables = [singable_event_table(900 + b, n) for b, n in enumerate([30, 12, 30])]
    counts = [capi.tracks_frame_count(tc, capi.events_from_table(t)) for t in tables]
    cut = min(counts[0], counts[2]) - 7
    assert cut > counts[1]
    for plan in (male_plan(precision=capi.PRECISION_F32), male_plan(delay=3), male5_plan()):
        stride = plan.output_capacity(cut)
        chain, entry, _ = events_chain_and_entry(plan, tc, tables, cut, stride, fresh_drift(3), maxabs=False)
        assert chain.frames.cpu().tolist() == counts and entry.frames.cpu().tolist() == counts
        fin = torch.isfinite(chain.audio).all(dim=1)
        assert bool(fin.any())
        assert torch.equal(chain.audio[fin].view(torch.int32), entry.audio[fin].view(torch.int32))
        assert torch.equal(chain.frames, entry.frames) and torch.equal(chain.counts, entry.counts)
        assert torch.equal(chain.drift.view(torch.int64), entry.drift.view(torch.int64))
        assert entry.counts[0].item() == plan.output_count(cut) and entry.counts[1].item() == plan.output_count(counts[1])


@pytest.mark.parametrize("precision", [capi.PRECISION_F32, capi.PRECISION_F64], ids=["f32", "f64"])
def test_events_entry_keeps_its_frames_while_a_host_entry_runs(precision):
    """gvtm_synthesize_events_device only enqueues.  A host entry called on the same plan while its kernels are still
    queued (other frames, more of them per utterance: the host entry grows its own staging and the noise-sample table)
    must leave the events entry's frames and tables alone: both calls come out bit for bit as each does alone."""
    import torch
    import tracks
    cfgv = np.array([4, 1, 1, 1, 1, -20.0, -6.0, 4.0, 250.0, 4.0])
    tc = product_config(cfgv)
    pool = [singable_event_table(700 + b, n) for b, n in enumerate([40, 25, 60, 33])]
    batch = 4096  # some milliseconds of synthesis: the host entry is called long before it is done
    max_frames = max(capi.tracks_frame_count(tc, capi.events_from_table(t)) for t in pool)
    d_events, d_offsets = events_on_device([pool[b % len(pool)] for b in range(batch)])
    dev = d_events.device
    plan = male_plan(precision=precision)
    stride = plan.output_capacity(max_frames)
    host_params = tracks.random_tracks(64, 2 * max_frames, seed0=17, consonant_heavy=True)
    side = torch.cuda.Stream()  # a non-blocking stream: nothing orders it against the host entry's own streams

    def enqueue_events():
        a = torch.zeros((batch, stride), dtype=torch.float32, device=dev)
        f = torch.zeros(batch, dtype=torch.int32, device=dev)
        n = torch.zeros(batch, dtype=torch.int64, device=dev)
        m = torch.zeros(batch, dtype=torch.float32, device=dev)
        side.wait_stream(torch.cuda.current_stream())
        plan.synthesize_events_device(tc, d_events, d_offsets, batch, max_frames, a, stride, f, n, m, None, side.cuda_stream)
        return a, f, n, m

    both = enqueue_events()
    host_both = plan.synthesize_host(host_params)  # no synchronisation in between
    torch.cuda.synchronize()
    alone = enqueue_events()
    torch.cuda.synchronize()
    host_alone = plan.synthesize_host(host_params)
    for x, y in zip(both, alone):  # samples, frame counts, sample counts, peaks: bit for bit
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    for x, y in zip(host_both, host_alone):
        assert x.tobytes() == y.tobytes()
