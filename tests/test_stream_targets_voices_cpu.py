"""Streams fed parameter targets under a mix of voices, without a device: the two entries' names in the header, the library
and the binding; their refusal of a null stream; the host rule under voice v (gvtm_targets_apply_host_from) resumed at the
cuts the GPU tests use, which makes it the oracle of those cuts; and the case module's sessions held to what they claim
(stream_targets_voices_cases.covers), each voice by its OWN filter length."""
import os
import re

import numpy as np
import pytest

import gama_tts_amd as g
from gama_tts_amd import capi
import stream_targets_cases as sessions
import stream_targets_voices_cases as sv
import targets5_voices_cases as cases5v
from targets_cases import spoken_lists
import voices_matrix_cases
from voice_cases import configs, male_plan

ENTRIES = ("gvtm_stream_push_targets_voices", "gvtm_stream_push_targets_model5_voices")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT = 1
F32_CHUNKS = {1: 144, 2: 96, 4: 48}  # the float shapes' chunks at SectionDelay 1, by rows


def voices_plan(names, precision=capi.PRECISION_F32):
    return g.VoicesPlan(configs(44100.0, 1, precision, names=names), 250.0, capi.DEVICE_NONE)


def one_row_chunk(precision):
    plan = male_plan(precision=precision, rows=1, device=capi.DEVICE_NONE)
    return int(plan._lib.gvtm_debug_chunk_length(plan._h, 1))


def test_the_entries_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "gama_vtm.h")).read()
    exports = open(os.path.join(ROOT, "gama_tts_amd", "csrc", "exports_vtm.map")).read()
    assert "global: gvtm_*;" in exports  # (the export list: every gvtm_ name, so the two below)
    lib = g.load_library()
    for name in ENTRIES:
        assert "int %s(gvtm_stream* stream, const int64_t* list_offsets" % name in header, name
        assert name in capi.PROTOTYPES and capi.PROTOTYPES[name] == capi.PROTOTYPES["gvtm_stream_push_targets"], name
        assert getattr(lib, name) is not None, name
    assert callable(g.Stream.push_targets_voices) and callable(g.Stream.push_targets_model5_voices)
    # both documents name the entries, and their "Not there" sentences no longer name streams of targets under several voices
    for document in ("README.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, document)).read()
        assert ENTRIES[0] in text and ENTRIES[1] in text, document
        not_there = [m.end() for m in re.finditer(r"\*?Not there\*?:", text)]
        assert not_there, document
        for at in not_there:
            assert "streams of targets" not in " ".join(text[at: at + 400].split()), document


@pytest.mark.parametrize("name", ENTRIES)
def test_a_null_stream_is_refused(name):
    lib = g.load_library()
    offsets = np.zeros(17, np.int64)
    assert getattr(lib, name)(None, capi._ptr(offsets), None, None, None, 0, None, 0, None, None) == INVALID_ARGUMENT
    assert b"null stream" in lib.gvtm_last_error()


def resumed_equals_whole(plan, voice, lists, pieces):
    n, total = plan.targets_filter_length(voice), sum(pieces)
    whole, status = capi.targets_apply_host(plan, lists, total, voice=voice)
    assert status == 0
    first, sums = 0, np.zeros(16)
    for count in pieces:
        # (what a stream holds in front of the piece: the points its voice's rule still needs)
        frames, sums, status = capi.targets_apply_host_from(plan, sessions.forget(lists, first, n), first, count, sums, voice=voice)
        assert status == 0 and frames.tobytes() == whole[first: first + count].tobytes(), (voice, first, count)
        first += count


def test_the_host_rule_under_a_voice_resumes_at_the_cuts():
    # the models 0 to 4: granule 12, the float one-row chunk
    plan = voices_plan(["male", "baby"])
    n = [plan.targets_filter_length(v) for v in range(2)]
    assert n[0] != n[1]
    for v in range(2):
        total = 3 * n[v] + 144 + 5
        resumed_equals_whole(plan, v, spoken_lists(total, 5 + v, wide=v == 1), sv.full_pieces(sv.GRANULE, 144, n[v], total))
    # model 5: granule 4, the chunk of 60
    plan5 = cases5v.voices_plan(True, names=["male", "baby"])
    n5 = [plan5.targets_filter_length(v) for v in range(2)]
    assert n5[0] == cases5v.MALE_N and n5[1] > 2 * n5[0]
    for v in range(2):
        total = 2 * n5[v] + 60 + 5
        lists = spoken_lists(total, 8 + v)
        resumed_equals_whole(plan5, v, lists, sv.chunk_pieces5(60, n5[v], total))
        resumed_equals_whole(plan5, v, lists, sv.window_pieces(sv.GRANULE5, n5[v], n5[v] + 1))
    # ... and the filters differ: a list trimmed by the shorter window is not what the longer one needs
    trimmed = sessions.forget(spoken_lists(3 * n5[1], 3), n5[1] + 400, n5[0])
    assert trimmed != sessions.forget(spoken_lists(3 * n5[1], 3), n5[1] + 400, n5[1])


def test_the_sessions_of_the_models_0_to_4_cover_every_voice():
    plan = voices_plan(["male", "female", "baby"])
    n = [plan.targets_filter_length(v) for v in range(3)]
    assert len(set(n)) == 3
    ids = (2, 0, 1, 0, 2)
    for precision in (capi.PRECISION_F32, capi.PRECISION_MIXED, capi.PRECISION_F64):
        chunk = one_row_chunk(precision)
        assert precision != capi.PRECISION_F32 or chunk == F32_CHUNKS[1]
        totals, pieces = sv.ragged_sessions(n, chunk, ids)
        assert totals[3] == 0 and not pieces[3] and 0 in pieces[1]
        for b, v in enumerate(ids):
            assert totals[b] <= 3 * n[v] + chunk + 5
        for v in range(3):
            mine = [pieces[b] for b in range(5) if ids[b] == v and pieces[b]]
            assert sv.covers(mine, sv.GRANULE, [chunk], n[v]), (precision, v)
            assert max(sv.resumes(p, sv.GRANULE) for p in mine) >= 2 and max(sum(p) for p in mine) > n[v]


@pytest.mark.parametrize("name,names,precision,rows,launched,chunk", sv.LOCKSTEP, ids=[c[0] for c in sv.LOCKSTEP])
def test_the_lockstep_sessions_cover_every_voice(name, names, precision, rows, launched, chunk):
    plan = g.VoicesPlan(configs(44100.0, 1, precision, names=list(names)), 250.0, capi.DEVICE_NONE, diagnostics=True, rows=rows)
    ids = sv.LOCKSTEP_IDS[rows]
    assert len(ids) <= 13 and voices_matrix_cases.stream_launch_shape(plan, len(ids))[0] == launched
    # (the chunk of the shape that is launched: the one-voice plan's forced to those rows)
    one_voice = male_plan(precision=precision, rows=launched, device=capi.DEVICE_NONE)
    assert int(one_voice._lib.gvtm_debug_chunk_length(one_voice._h, 13)) == chunk
    n = [plan.targets_filter_length(v) for v in range(3)]
    totals, pieces = sv.lockstep_sessions(n, chunk, ids)
    for b, v in enumerate(ids):
        assert totals[b] <= 3 * n[v] + chunk + 5 and sv.covers([pieces[b]], sv.GRANULE, [chunk], n[v]) and sv.resumes(pieces[b], sv.GRANULE) >= 2
    # lockstep per voice: the utterances of a voice are pushed the same pieces, those of different voices are not
    assert all((pieces[a] == pieces[b]) == (ids[a] == ids[b]) for a in range(len(ids)) for b in range(len(ids)))


@pytest.mark.parametrize("float_class,chunk", [(True, 60), (True, 52), (False, 56)], ids=["float-chunk60", "float-chunk52", "double-chunk56"])
def test_the_sessions_of_model_5_cover_every_voice(float_class, chunk):
    plan = cases5v.voices_plan(float_class)
    n = [plan.targets_filter_length(v) for v in range(5)]
    longest = max(cases5v.CHUNKS[float_class])
    by_name = sv.model5_sessions(n, chunk, longest)
    ids = sv.MODEL5_IDS
    assert len(ids) <= 13 and sv.no_own_index(ids)
    fixture_cases = set(cases5v.all_cases(plan, float_class))
    for totals, pieces in by_name.values():
        # in lockstep per voice, which is what lets the stream launch the forced shape (the chunk the pieces sit around)
        assert sv.in_lockstep_per_voice(sv.schedule_of(pieces), ids)
        for v, total, p in zip(ids, totals, pieces):
            assert sum(p) == total <= 2 * n[v] + longest + 5
            assert v == 0 or (cases5v.VOICES[v], total) in fixture_cases, (v, total)
    for v in range(5):
        mine = [p for _, pieces in by_name.values() for w, p in zip(ids, pieces) if w == v]
        assert sv.covers(mine, sv.GRANULE5, [chunk], n[v]), v
        assert max(sv.resumes(p, sv.GRANULE5) for p in mine) >= 2


def test_the_lockstep_rule_tells_a_ragged_schedule():
    assert sv.in_lockstep_per_voice([[5, 7, 5], [0, 1, 0]], (1, 0, 1))
    assert not sv.in_lockstep_per_voice([[5, 7, 5], [0, 1, 4]], (1, 0, 1))
    n = [1002, 1169, 2337]
    assert not sv.in_lockstep_per_voice(sv.schedule_of(sv.ragged_sessions(n, 144)[1]), (2, 0, 1, 0, 2))


def test_reading_the_sums_asks_for_a_diagnostics_plan():
    stream = g.Stream.__new__(g.Stream)  # (no device here: the guard stands in front of the library call)
    stream._plan, stream._h, stream.batch = cases5v.voices_plan(True), None, 1
    with pytest.raises(ValueError, match="diagnostics"):
        stream.targets_sums()
