"""The several-voices variant of every shape of vtm_synth_kernel a launch can be forced to, on the device.

vtm_synth_kernel is compiled twice per shape: for one voice, and with kVoicesFlag for a launch that mixes voices.  The
voice variant picks its utterances through the row map, ends a voice's groups with empty rows, takes its voice's constants
and wavetable, computes its own ring length inside an LDS sized for the longest ring of the launch, and as a stream
carries its own chunk argument and state stride.  test_gpu_shape_matrix.py holds the single-voice kernels down on every
shape; this file does the same for the voice variant: the 113 cells of voices_matrix_cases.py that launch with the rows
forced on them (precision x tube x mix of voices x rows), each in

    launch A    19 or 30 ragged utterances of two or three voices, shuffled, every voice with 0, 1 and 2 frames and lengths
                on the three last-chunk residues of ITS steps per frame, its last group partly empty, into a buffer filled
                with a sentinel: every count is gvtm_voice_output_count and the oracle's; samples and maxabs bit for bit
                those of a single-voice plan of that voice forced to the launched rows (include/gama_vtm.h's contract);
                samples within parity_rules.TOL of the oracle (float: bit-identical); the row untouched beyond its count;
                all samples finite; copies of a track bit for bit their first occurrence;
    launch B    seven utterances, none of voice 0, ids -1 and n_voices among them: the bad ids give out_counts -1, maxabs 0
                and an untouched row, all others what the same utterances give in a launch without the bad ids;
    a stream    rows + 1 utterances of every voice pushed in lockstep in uneven pieces: samples, counts and maxabs bit for
                bit the one-shot voices launch of the same utterances (float: the float oracle as well), held to the rows
                gvtm_debug_stream_launch_shape answers (VOICES_STREAM_FALL_BACK launch as two rows).

tests/test_voices_matrix_cases.py (CPU) shows that the comparison discriminates: no two utterances of launch A that are
not copies have equal expected samples, and one track gives different samples under each pair of voices."""
import numpy as np
import pytest

from device_io import run_voices_device
from gama_tts_amd import capi
from parity_rules import TOL, peak_err, within
from shape_matrix_cases import STREAM_FRAMES, STREAM_PIECES
from voice_cases import push_in_pieces
from voices_matrix_cases import (BATCH_B, CELLS, LAUNCHABLE, SENTINEL, VOICES_FALL_BACK, VOICES_STREAM_FALL_BACK, batch_a,
                                 cell_id, launch_a, launch_b, oracle_many, oracle_pools, rows_of, single_plan, stream_case,
                                 stream_launch_shape, stream_rows, upsampling_of, voices_launch_shape, voices_plan)

pytestmark = pytest.mark.gpu

IDS = [cell_id(c) for c in LAUNCHABLE]
each_cell = pytest.mark.parametrize("cell", LAUNCHABLE, ids=IDS)
STREAM_IDS = [cell_id(c) + ("-as-rows2" if cell_id(c) in VOICES_STREAM_FALL_BACK else "") for c in LAUNCHABLE]
each_stream = pytest.mark.parametrize("cell", LAUNCHABLE, ids=STREAM_IDS)


def _singles(cell, params, ids, frames, rows):
    """Every utterance through a single-voice plan of its voice forced to `rows` -> {b: (samples, count, maxabs)}."""
    out = {}
    for v in range(len(cell.names)):
        sel = np.flatnonzero(ids == v)
        if sel.size == 0:
            continue
        plan = single_plan(cell, v, rows)
        assert plan.info.upsampling == upsampling_of(cell)[v]
        audio, counts, maxabs = plan.synthesize_host(params[sel], frames[sel])
        for j, b in enumerate(sel):
            out[int(b)] = (audio[j, : counts[j]], int(counts[j]), maxabs[j])
        plan.close()
    return out


@each_cell
def test_launch_a_every_voice_on_its_chunk_residues(cell):
    plan = voices_plan(cell)
    a = launch_a(cell, plan)
    batch = a.ids.size
    assert batch == batch_a(cell) and voices_launch_shape(plan, batch)[0] == rows_of(cell) == cell.rows
    stride = plan.voices_output_capacity(a.params.shape[1])
    audio, counts, maxabs = run_voices_device(plan, a.params, a.ids, a.frames, stride, fill=SENTINEL)
    singles = _singles(cell, a.params, a.ids, a.frames, cell.rows)
    refs = oracle_pools(cell, a)
    first = {}
    for b in range(batch):
        v, n = int(a.ids[b]), int(counts[b])
        ref = refs[a.member[b]]
        got = audio[b, :n]
        print("%s utterance %2d voice %d frames %2d count %6d peak error %.3g"
              % (cell_id(cell), b, v, a.frames[b], n, peak_err(got, ref) if ref.size == n and n else 0.0))
        assert n == plan.voice_output_count(v, int(a.frames[b])) == ref.size, (b, v, int(a.frames[b]), n, ref.size)
        s_audio, s_n, s_max = singles[b]
        assert n == s_n and np.array_equal(got, s_audio), (b, v, int(a.frames[b]))
        assert maxabs[b] == s_max == (np.abs(got).max() if n else 0.0), (b, v, maxabs[b], s_max)
        assert within(got, ref, TOL[cell.precision]), (b, v, int(a.frames[b]), peak_err(got, ref))
        assert (audio[b, n:] == SENTINEL).all(), (b, v, n)  # the row is untouched beyond its count
        assert np.isfinite(got).all() and np.isfinite(maxabs[b]), b
        at = first.setdefault(a.member[b], b)
        assert counts[b] == counts[at] and maxabs[b] == maxabs[at] and np.array_equal(audio[b], audio[at]), (b, at)
    assert len(first) < batch  # (there are copies)


@each_cell
def test_launch_b_a_voice_without_utterances_and_bad_ids(cell):
    plan = voices_plan(cell)
    n_voices = len(cell.names)
    b_case = launch_b(cell, launch_a(cell, plan))
    assert b_case.bad_ids.size == BATCH_B and not (b_case.bad_ids == 0).any() and not (b_case.good_ids == 0).any()
    bad = np.flatnonzero(b_case.bad_ids != b_case.good_ids)
    assert sorted(b_case.bad_ids[bad].tolist()) == [-1, n_voices]
    stride = plan.voices_output_capacity(b_case.params.shape[1])
    good_audio, good_counts, good_max = run_voices_device(plan, b_case.params, b_case.good_ids, b_case.frames, stride, fill=SENTINEL)
    audio, counts, maxabs = run_voices_device(plan, b_case.params, b_case.bad_ids, b_case.frames, stride, fill=SENTINEL)
    for b in range(BATCH_B):
        if b in bad:
            assert counts[b] == -1 and maxabs[b] == 0.0 and (audio[b] == SENTINEL).all(), (b, counts[b], maxabs[b])
        else:
            v = int(b_case.good_ids[b])
            assert counts[b] == good_counts[b] == plan.voice_output_count(v, int(b_case.frames[b])) > 0, (b, v, counts[b])
            assert maxabs[b] == good_max[b] > 0.0, (b, v)
            assert np.array_equal(audio[b], good_audio[b]), (b, v)
            assert (audio[b, counts[b]:] == SENTINEL).all() and np.isfinite(audio[b, : counts[b]]).all(), (b, v)


@each_stream
def test_stream_in_lockstep_is_the_one_shot_voices_launch(cell):
    plan = voices_plan(cell)
    params, ids = stream_case(cell)
    batch = ids.size
    rows, ring, lds = stream_launch_shape(plan, batch)
    assert rows == stream_rows(cell) and batch == (rows + 1) * len(cell.names) and lds <= 160 * 1024, (rows, ring, lds)
    total = np.full(batch, STREAM_FRAMES, dtype=np.int32)
    whole, counts, maxabs = plan.synthesize_host(params, ids)
    outs, peaks = push_in_pieces(plan, params, total, STREAM_PIECES, voice_ids=ids)
    for b in range(batch):
        assert outs[b].size == counts[b] == plan.voice_output_count(int(ids[b]), STREAM_FRAMES) > 0, (b, outs[b].size, counts[b])
        assert np.array_equal(outs[b], whole[b, : counts[b]]), (b, int(ids[b]))
        assert peaks[b] == maxabs[b] == np.abs(whole[b]).max(), (b, int(ids[b]))
    if cell.precision == capi.PRECISION_F32:
        refs = oracle_many(cell, [(int(ids[b]), params[b]) for b in range(batch)])
        for b in range(batch):
            assert np.array_equal(outs[b], refs[b]), (b, int(ids[b]))


def test_the_matrix_is_complete():
    """The parametrization above is the whole table: of the 135 cells the 113 that keep their forced rows, each once and
    none skipped; the other 22 launch as two rows -- and are exactly the ones the table names; the streams that launch as
    two rows are the ones the library's hook names."""
    assert len(CELLS) == 135 and len(set(CELLS)) == 135
    keeps, stream_falls = set(), set()
    for c in CELLS:
        plan = voices_plan(c, capi.DEVICE_NONE)
        if voices_launch_shape(plan, batch_a(c))[0] == c.rows:
            keeps.add(cell_id(c))
            if stream_launch_shape(plan, (c.rows + 1) * len(c.names))[0] != c.rows:
                stream_falls.add(cell_id(c))
        plan.close()
    assert len(keeps) == 113 and keeps == set(IDS) and len(IDS) == 113
    assert {cell_id(c) for c in CELLS} - keeps == VOICES_FALL_BACK and len(VOICES_FALL_BACK) == 22
    assert stream_falls == VOICES_STREAM_FALL_BACK
    for fn in (test_launch_a_every_voice_on_its_chunk_residues, test_launch_b_a_voice_without_utterances_and_bad_ids,
               test_stream_in_lockstep_is_the_one_shot_voices_launch):
        marks = [m for m in fn.pytestmark if m.name == "parametrize"]
        assert len(marks) == 1 and [cell_id(c) for c in marks[0].args[1]] == IDS
        assert not [m for m in fn.pytestmark if m.name in ("skip", "skipif", "xfail")]
