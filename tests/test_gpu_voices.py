"""Several voices in one batched launch (gvtm_plan_create_voices + gvtm_synthesize_voices_*).

The five GamaTTS variants of data/voice/english/0_male (tests/golden/voice_*.txt: vocal tract 17.5 / 15 / 12.5 / 10 /
7.5 cm) mixed in one batch, ids interleaved and ragged.  Every utterance must come out bit for bit as a single-voice plan
of its voice synthesizes it in the same workgroup shape, and within the parity tests' tolerances of the oracle (float:
bit-identical).  The grouping kernel (a stable counting sort by voice, each voice padded to whole workgroups) is checked
on its own against a numpy restatement."""
import numpy as np
import pytest

import gama_tts_amd as g
from gama_tts_amd import capi
import oracle
import tracks
from device_io import run_voices_device
from parity_rules import TOL, within
from voice_cases import CASE_IDS, CASES, configs, mixed_batch, oracle_config
from voice_files import VOICES

pytestmark = pytest.mark.gpu


def singles_of(cfgs, params, ids, frames, diagnostics=False, rows=0):
    """Every utterance through a single-voice plan of its voice: the same batch (same workgroup shape), that voice's rows kept."""
    out = {}
    for v, cfg in enumerate(cfgs):
        sel = np.nonzero(ids == v)[0]
        if sel.size == 0:
            continue
        p = g.Plan(cfg, 250.0, 0, diagnostics=diagnostics, rows=rows)
        pad = np.zeros(len(ids) - sel.size, dtype=np.intp)  # filler utterances: keep the batch size, hence the shape
        idx = np.concatenate([sel, pad])
        audio, counts, maxabs = p.synthesize_host(params[idx], frames[idx])
        for j, b in enumerate(sel):
            out[int(b)] = (audio[j, : counts[j]], int(counts[j]), float(maxabs[j]))
    return out


@pytest.mark.parametrize("precision,delay,rate,layout", CASES, ids=CASE_IDS)
def test_five_voices_in_one_launch(precision, delay, rate, layout):
    cfgs = configs(rate, delay, precision, layout)
    plan = g.VoicesPlan(cfgs, 250.0, 0)
    params, ids, frames = mixed_batch(48, 30, 5, seed=11 + delay + 3 * precision + 7 * layout)
    stride = plan.voices_output_capacity(params.shape[1])
    audio, counts, maxabs = run_voices_device(plan, params, ids, frames, stride)
    singles = singles_of(cfgs, params, ids, frames)
    for b in range(len(ids)):
        v = int(ids[b])
        n = int(counts[b])
        assert n == plan.voice_output_count(v, int(frames[b])), b
        ref_audio, ref_n, ref_max = singles[b]
        assert n == ref_n and np.array_equal(audio[b, :n], ref_audio), (b, v, int(frames[b]))
        assert maxabs[b] == ref_max
        want = oracle.synthesize(oracle_config(VOICES[v], rate, delay, layout, precision), params[b, : frames[b]])
        assert want.size == n
        if n:
            assert within(audio[b, :n], want, TOL[precision]), (b, v)
    # the voices differ: the same track of two voices does not give the same samples
    assert plan.voice_output_count(0, 30) != plan.voice_output_count(4, 30)


@pytest.mark.parametrize("precision", [capi.PRECISION_F32, capi.PRECISION_F64], ids=["f32", "f64"])
def test_uneven_voices_in_four_row_workgroups(precision):
    """One voice with a single utterance, another with U + 1 = 5: workgroups of four rows, partly empty."""
    cfgs = configs(precision=precision, names=["male", "female"])
    plan = g.VoicesPlan(cfgs, 250.0, 0, diagnostics=True, rows=4)
    ids = np.array([1, 1, 0, 1, 1, 1], dtype=np.int32)
    params = tracks.random_tracks(6, 20, seed0=321, consonant_heavy=True)
    frames = np.array([20, 7, 13, 1, 0, 19], dtype=np.int32)
    stride = plan.voices_output_capacity(20)
    audio, counts, maxabs = run_voices_device(plan, params, ids, frames, stride)
    singles = singles_of(cfgs, params, ids, frames, diagnostics=True, rows=4)
    for b in range(6):
        ref_audio, ref_n, ref_max = singles[b]
        assert counts[b] == ref_n and np.array_equal(audio[b, : ref_n], ref_audio), b
        assert maxabs[b] == ref_max


def test_out_of_range_voice_ids_fail_alone():
    cfgs = configs(precision=capi.PRECISION_F32)
    plan = g.VoicesPlan(cfgs, 250.0, 0)
    params, ids, frames = mixed_batch(24, 16, 5, seed=5)
    bad = ids.copy()
    bad[[3, 10, 17]] = [-1, 5, 1 << 20]
    stride = plan.voices_output_capacity(16)
    good_audio, good_counts, good_max = run_voices_device(plan, params, ids, frames, stride)
    audio, counts, maxabs = run_voices_device(plan, params, bad, frames, stride, fill=7.0)
    for b in range(24):
        if b in (3, 10, 17):
            assert counts[b] == -1 and maxabs[b] == 0.0
            assert (audio[b] == 7.0).all()  # the device entry leaves the row untouched
        else:
            n = int(good_counts[b])
            assert counts[b] == n and maxabs[b] == good_max[b]
            assert np.array_equal(audio[b, :n], good_audio[b, :n])
    # the host entries: the row comes back zero
    h_audio, h_counts, h_max = plan.synthesize_host(params, bad, frames)
    assert (h_counts[[3, 10, 17]] == -1).all() and not h_audio[[3, 10, 17]].any() and not h_max[[3, 10, 17]].any()
    keep = np.setdiff1d(np.arange(24), [3, 10, 17])
    assert np.array_equal(h_counts[keep], good_counts[keep])
    for b in keep:
        n = int(good_counts[b])
        assert np.array_equal(h_audio[b, :n], good_audio[b, :n]) and not h_audio[b, n:].any()
    pcm, p_counts, p_max, scales = plan.synthesize_host_pcm16(params, bad, frames)
    assert (p_counts[[3, 10, 17]] == -1).all() and not pcm[[3, 10, 17]].any() and not scales[[3, 10, 17]].any()


@pytest.mark.parametrize("precision", [capi.PRECISION_F32, capi.PRECISION_F64], ids=["f32", "f64"])
def test_host_entries_slice_a_big_mixed_batch(precision):
    """Two machine-fulls and more (four per workgroup x 256 compute units = 1024): the host pipeline cuts the batch into
    slices, each with its own grouping.  Float and pcm16 host entries against the device entry in one launch."""
    import torch
    cfgs = configs(precision=precision)
    plan = g.VoicesPlan(cfgs, 250.0, 0)
    pool, batch, max_frames = 40, 2600, 12
    pp, pids, pf = mixed_batch(pool, max_frames, 5, seed=77)
    idx = np.random.default_rng(3).integers(0, pool, size=batch)
    params, ids, frames = pp[idx], pids[idx], pf[idx]
    stride = plan.voices_output_capacity(max_frames)
    d_audio, d_counts, d_max = run_voices_device(plan, params, ids, frames, stride)
    for b in range(batch):  # ragged rows: zero beyond the count only in the host entries; compare the counted part
        assert d_counts[b] == plan.voice_output_count(int(ids[b]), int(frames[b]))
    audio, counts, maxabs = plan.synthesize_host(params, ids, frames)
    assert np.array_equal(counts, d_counts) and np.array_equal(maxabs, d_max)
    for b in range(batch):
        n = int(counts[b])
        assert np.array_equal(audio[b, :n], d_audio[b, :n]) and not audio[b, n:].any(), b
    # copies of one pool track are identical wherever they landed
    first = {}
    for b in range(batch):
        first.setdefault(int(idx[b]), b)
        a = first[int(idx[b])]
        assert np.array_equal(audio[b], audio[a])
    pcm, p_counts, p_max, scales = plan.synthesize_host_pcm16(params, ids, frames)
    assert np.array_equal(p_counts, d_counts) and np.array_equal(p_max, d_max)
    # pcm16 = gvtm_normalize_batch_device of the device entry's samples
    da = torch.from_numpy(np.ascontiguousarray(np.where(np.arange(stride)[None, :] < d_counts[:, None], d_audio, 0.0).astype(np.float32))).cuda()
    dc = torch.from_numpy(d_counts).cuda()
    dm = torch.from_numpy(d_max).cuda()
    di16 = torch.zeros((batch, stride), dtype=torch.int16, device="cuda")
    ds = torch.zeros(batch, dtype=torch.float32, device="cuda")
    for q in range(0, batch, 32768):
        m = min(32768, batch - q)
        plan.normalize_device(da[q:], m, stride, dm[q:], dc[q:], None, di16[q:], ds[q:], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(pcm, di16.cpu().numpy())
    assert np.array_equal(scales, ds.cpu().numpy())


@pytest.mark.parametrize("precision", [capi.PRECISION_F32, capi.PRECISION_F64], ids=["f32", "f64"])
def test_device_entry_keeps_its_grouping_while_a_host_entry_runs(precision):
    """gvtm_synthesize_voices_device only enqueues.  The voices host entry called on the same plan while its kernels are
    still queued (other utterances, more frames each) groups its own batch in scratch of its own: both calls come out bit
    for bit as each does alone."""
    import torch
    plan = g.VoicesPlan(configs(precision=precision), 250.0, 0)
    batch, max_frames = 4096, 250  # some milliseconds of synthesis: the host entry is called long before it is done
    params, ids, frames = mixed_batch(batch, max_frames, 5, seed=91)
    h_params, h_ids, h_frames = mixed_batch(64, 2 * max_frames, 5, seed=92)
    stride = plan.voices_output_capacity(max_frames)
    dp, di, df = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (params, ids, frames))
    side = torch.cuda.Stream()  # a non-blocking stream: nothing orders it against the host entry's own streams

    def enqueue_device():
        da = torch.zeros((batch, stride), dtype=torch.float32, device="cuda")
        dc = torch.zeros(batch, dtype=torch.int64, device="cuda")
        dm = torch.zeros(batch, dtype=torch.float32, device="cuda")
        side.wait_stream(torch.cuda.current_stream())
        plan.synthesize_voices_device(dp, di, batch, max_frames, da, stride, df, dc, dm, side.cuda_stream)
        return da, dc, dm

    both = enqueue_device()
    host_both = plan.synthesize_host(h_params, h_ids, h_frames)  # no synchronisation in between
    torch.cuda.synchronize()
    alone = enqueue_device()
    torch.cuda.synchronize()
    host_alone = plan.synthesize_host(h_params, h_ids, h_frames)
    for x, y in zip(both, alone):  # samples, sample counts, peaks: bit for bit
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    for x, y in zip(host_both, host_alone):
        assert x.tobytes() == y.tobytes()


def _numpy_grouping(ids, n_voices, rows):
    groups = (len(ids) + rows - 1) // rows + n_voices
    row_map = np.full(groups * rows, -1, dtype=np.int32)
    group_voice = np.full(groups, -1, dtype=np.int32)
    g0 = 0
    for v in range(n_voices):
        members = np.nonzero(ids == v)[0]  # stable: in batch order
        ng = (members.size + rows - 1) // rows
        row_map[g0 * rows: g0 * rows + members.size] = members
        group_voice[g0: g0 + ng] = v
        g0 += ng
    return row_map, group_voice


@pytest.mark.parametrize("rows", [1, 2, 4])
def test_grouping_kernel_is_a_stable_counting_sort(rows):
    import torch
    plan = g.VoicesPlan(configs(precision=capi.PRECISION_F32), 250.0, 0, diagnostics=True)
    rng = np.random.default_rng(rows)
    lists = [
        np.full(1000, 4, dtype=np.int32),                                  # one voice only (the last)
        np.tile(np.arange(5, dtype=np.int32), 401),                        # round robin
        np.repeat(np.array([4, 3, 2, 1, 0], dtype=np.int32), [1, 257, 3, 0, 700]),  # runs, reversed, a voice without any
        rng.integers(-2, 7, size=3001).astype(np.int32),                   # random, with ids out of range
        np.array([2], dtype=np.int32),                                     # a batch of one
        np.concatenate([rng.integers(0, 5, size=777), [-1, 5, -2147483648, 2147483647]]).astype(np.int32),
    ]
    for ids in lists:
        batch = len(ids)
        groups = (batch + rows - 1) // rows + 5
        di = torch.from_numpy(ids).cuda()
        dmap = torch.full((groups * rows,), 123, dtype=torch.int32, device="cuda")
        dgv = torch.full((groups,), 123, dtype=torch.int32, device="cuda")
        dc = torch.zeros(batch, dtype=torch.int64, device="cuda")
        dm = torch.full((batch,), 9.0, dtype=torch.float32, device="cuda")
        plan._check(plan._lib.gvtm_debug_group_voices(plan._h, di.data_ptr(), batch, rows, dmap.data_ptr(), dgv.data_ptr(),
                                                      dc.data_ptr(), dm.data_ptr()))
        want_map, want_gv = _numpy_grouping(ids, 5, rows)
        assert np.array_equal(dmap.cpu().numpy(), want_map)
        assert np.array_equal(dgv.cpu().numpy(), want_gv)
        bad = (ids < 0) | (ids >= 5)
        assert (dc.cpu().numpy()[bad] == -1).all() and (dc.cpu().numpy()[~bad] == 0).all()
        assert (dm.cpu().numpy()[bad] == 0.0).all() and (dm.cpu().numpy()[~bad] == 9.0).all()
