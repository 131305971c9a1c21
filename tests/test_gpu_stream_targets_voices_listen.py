"""A targets-fed stream of several voices that listens (gvtm_stream_listen on a gvtm_stream_create_voices stream fed by
gvtm_stream_push_targets_voices): one session of two voices on a float plan of the models 0 to 4, no sample leaving the device
(`audio` NULL).  The bar is test_gpu_stream_listen.py's, equality of bits: each utterance's queued spectra and signal views
are the rows gvtm_analyze_spectrum_device writes for the same analysis object on the one-shot voices entry's row of that
utterance, which the stream contract makes the session's own samples.

The ring is 65 536 output samples, so this is the one test of the feature whose utterances are that long: one ring each
and a remainder."""
import numpy as np
import pytest

import analysis_cases as ac
import gama_tts_amd as g
from gama_tts_amd import capi
from targets_cases import spoken_lists
from targets_io import run_targets as one_shot_voices
from test_gpu_analysis import run_device
from test_gpu_stream_listen import Heard, analysis, same_views, targets_session
from voice_cases import configs

pytestmark = pytest.mark.gpu

N = ac.N


def steps_for(plan, voice, samples):
    """The fewest steps of an utterance of `voice` that finishes with at least `samples` samples."""
    lo, hi = 1, 400000
    while lo < hi:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if plan.targets_voice_output_count(voice, mid) >= samples else (mid + 1, hi)
    return lo


def test_a_listening_session_of_two_voices_equals_the_analysis_of_the_one_shot_rows():
    plan = g.VoicesPlan(configs(44100.0, 1, capi.PRECISION_F32, names=["male", "female"]), 250.0, 0)
    ids = [1, 0]
    n = [plan.targets_filter_length(v) for v in ids]
    assert n[0] != n[1]
    # one ring and a remainder each; the first pushes sit around the granule, the third carries most of the ring
    totals = [steps_for(plan, v, N) + 700 + 100 * b for b, v in enumerate(ids)]
    schedule = [[13, 25], [11, 0], [totals[0] - 500, totals[1] - 300], [476, 275]]
    assert [sum(col) for col in zip(*schedule)] == totals
    utterances = [spoken_lists(t, 90 + b) for b, t in enumerate(totals)]
    whole = one_shot_voices(plan, utterances, totals, ids)
    rows = [whole[0][b, : whole[1][b]].copy() for b in range(2)]
    assert all(N <= r.size < 2 * N for r in rows)
    an = analysis("blackman-log")
    want_spectra, want_signal, want_buffers = run_device(an, rows, None, 1)
    assert want_buffers.tolist() == [1, 1]
    stream = g.Stream(plan, 2, voice_ids=ids)
    stream.listen(an, 1, spectra=True, signal=True)
    heard = Heard(stream)
    counts, sizes = targets_session(stream, utterances, schedule, heard, audio=False, entry="push_targets_voices")
    assert counts == [r.size for r in rows]
    same_views(heard, want_spectra, want_signal, want_buffers)
    fill, queued = stream.listen_state()
    assert fill.tolist() == [r.size - N for r in rows] and not queued.any()
