"""What the tests of the targets-fed streams of several voices share (gvtm_stream_push_targets_voices,
gvtm_stream_push_targets_model5_voices): the sessions an utterance of voice v is cut into, with v's OWN filter length N_v,
and the rules their schedules are held to (targets_io.session drives them).  An utterance is 16 lists of (steps, values), as in
targets_cases.py.

A voice's sessions, between them, must have
  * pieces of 1, granule - 1, granule and granule + 1 steps (the granule: 12 steps, model 5: 4) -- what a push keeps pending;
  * pieces of chunk - 1, chunk and chunk + 1 steps for the chunk of every kernel shape the test launches -- a launch begins
    at chunk 0 whatever the utterance's step, so a piece's SIZE is what meets the chunk;
  * N_v - 1, N_v and N_v + 1, as a piece's size or as a cut (the step a push ends in front of): a piece of about N_v steps
    is a launch in which the leave cursor starts moving, a cut at about N_v a launch that resumes where the window has just
    filled.  All three as pieces do not fit the step budget (model 5: 2 N_v + chunk + 5 steps, else 3 N_v + chunk + 5): the
    models 0 to 4 have the three cuts and the sizes N_v - 1 and N_v + 1 in one session (full_pieces); model 5 has the size
    N_v - 1 in its long session (stream_targets5_cases.pieces5 with the voice's N) and the cuts in the session of N_v + 1 steps.
`covers` states this rule, and the CPU test holds every session of the GPU tests to it."""
import numpy as np

from stream_targets5_cases import pieces5

GRANULE, GRANULE5 = 12, 4


def full_pieces(granule, chunk, n, total):
    """The session of the models 0 to 4, `total` <= 3 n + chunk + 5 steps under a filter of n samples: cuts in front of the
    steps n - 1, n and n + 1, pieces around the granule and around the chunk, a piece of n + 1 steps, the rest."""
    out = [n - 1, 1, 1, granule - 1, granule, granule + 1, chunk - 1, chunk, chunk + 1, n + 1]
    assert total > sum(out), (total, sum(out))
    return out + [total - sum(out)]


def chunk_pieces5(chunk, n, total):
    """Model 5's long session: stream_targets5_cases.pieces5 with the voice's own n, its last piece stretched to `total` (the
    fixtures' long case is 2 n + 5 past the class's LONGEST chunk, whichever chunk is launched)."""
    out = pieces5(chunk, n)
    out[-1] += total - sum(out)
    assert out[-1] > 0
    return out


def window_pieces(granule, n, total):
    """The window session: cuts in front of the steps n - 1, n and n + 1, then pieces around the granule, then the rest (none
    where total == n + 1)."""
    out = [n - 1, 1, 1]
    assert total >= n + 1
    if total > n + 1:
        out += [granule - 1, granule, granule + 1]
        assert total > sum(out)
        out.append(total - sum(out))
    return out


def cuts(pieces):
    """The steps the pushes of a session end in front of."""
    return [int(c) for c in np.cumsum(pieces)]


def covers(voice_sessions, granule, chunks, n):
    """Do the sessions of one voice (lists of pieces) cover what the module's docstring asks of them?"""
    sizes = {int(p) for s in voice_sessions for p in s}
    marks = sizes | {c for s in voice_sessions for c in cuts(s)}
    around = lambda x: {x - 1, x, x + 1}  # noqa: E731
    return ({1} | around(granule)) <= sizes and all(around(c) <= sizes for c in chunks) and around(n) <= marks and bool(sizes & {n - 1, n, n + 1})


def resumes(pieces, granule):
    """The launches of a session that resume (begin behind step 0): a push launches when it brings the pending steps to a
    granule; the finish launches whatever is pending, or nothing."""
    pending, done, count = 0, 0, 0
    for p in list(pieces) + [None]:
        launch = pending if p is None else (pending + p) // granule * granule
        pending = 0 if p is None else pending + p - launch
        if launch and done:
            count += 1
        done += launch
    return count


def schedule_of(pieces_by_utterance):
    """Per-utterance pieces -> the pushes of a session, push i giving utterance b its i-th piece (0 once it has none left)."""
    pushes = max(len(p) for p in pieces_by_utterance)
    return [[int(p[i]) if i < len(p) else 0 for p in pieces_by_utterance] for i in range(pushes)]


def log_bound(lists, done, n):
    """The most points a stream may hold for an utterance with `done` steps given: those of its last n + 12 steps, and one
    more per list."""
    return sum(1 for steps, _ in lists for s in steps if done - (n + 12) <= s < done) + 16


def no_own_index(voice_ids):
    """The rule of targets_io.at_own_index, restated: the grouping is a stable sort by voice, one workgroup per
    utterance; is NO utterance left at the workgroup of its own index?"""
    return not [b for g, b in enumerate(sorted(range(len(voice_ids)), key=lambda b: voice_ids[b])) if g == b]


# ---- the sessions of the GPU tests, so that the CPU test can hold them to `covers` without a device ----

def ragged_sessions(n, chunk, ids=(2, 0, 1, 0, 2)):
    """tests/test_gpu_stream_targets_voices.py, a.: five utterances of three voices with filters n[v], one utterance per
    workgroup (the one-row chunk).  Utterance 3 is never pushed; utterance 1 receives a push of 0 steps in between; utterance
    4, the second of its voice, is cut elsewhere.  -> (totals, pieces per utterance)"""
    totals = [3 * n[v] + chunk + 5 for v in ids]
    totals[3], totals[4] = 0, 2 * n[ids[4]] + 77
    pieces = [full_pieces(GRANULE, chunk, n[v], t) if b < 3 else [] for b, (v, t) in enumerate(zip(ids, totals))]
    pieces[1].insert(4, 0)
    pieces[4] = [24, 7, n[ids[4]], n[ids[4]] + 46]
    assert [sum(p) for p in pieces] == totals
    return totals, pieces


# (name, voices, precision (capi.PRECISION_*: 2 float, 1 mixed), forced rows, the rows a stream of the plan launches, that
# shape's chunk).  A stream keeps the one-row shape's ring whatever it launches, and the voice variant's LDS is sized for the
# longest of the voices': in float four forced rows launch as two beside any voice, and it is the mixed precision, with its
# chunk of 32, whose streams of up-sampling voices run four rows.
LOCKSTEP = [("f32-rows2", ("male", "female", "baby"), 2, 2, 2, 96), ("f32-rows4-as-2", ("male", "female", "baby"), 2, 4, 2, 96),
            ("mixed-rows4", ("male", "female", "large_child"), 1, 4, 4, 32)]
LOCKSTEP_IDS = {2: (2, 0, 1, 0, 2, 1, 0), 4: (0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2, 0)}


def lockstep_sessions(n, chunk, ids):
    """... a., lockstep per voice: every utterance of voice v is pushed v's pieces -> (totals, pieces per utterance).  (The
    shape hook gvtm_debug_stream_launch_shape answers for a lockstep stream: it is this schedule's being in lockstep per voice
    that makes its answer the shape the stream launches.)"""
    pieces = [full_pieces(GRANULE, chunk, n[v], 3 * n[v] + chunk + 5) for v in ids]
    assert in_lockstep_per_voice(schedule_of(pieces), ids)
    return [sum(p) for p in pieces], pieces


def in_lockstep_per_voice(schedule, ids):
    """The rule by which a stream lets its utterances share a launch's FORCED shape (csrc/vtm_capi_stream.cpp: stream_launch):
    in every push, every utterance of a voice is given what the voice's first utterance is given -- so the utterances of a voice
    synthesize the same steps from the same step in every launch.  A session that is not launches one utterance per
    workgroup in the one-row shape (model 5: its index 0) whatever the plan forces, and a test that names a forced shape must
    hold its schedule to this."""
    first = {v: list(ids).index(v) for v in set(ids)}
    return all(push[b] == push[first[v]] for push in schedule for b, v in enumerate(ids))


MODEL5_IDS = (4, 1, 2, 2, 3, 0, 4, 0, 3, 1)  # every voice twice, no utterance at its workgroup's own index


def model5_sessions(n, chunk, longest):
    """tests/test_gpu_stream_targets5_voices.py, a. and b.: three sessions of MODEL5_IDS on the five-voice plan with filters
    n[v], each in lockstep per voice, so that the stream launches the shape the plan forces: under voice v both utterances
    have the session's case of the fixtures -- "long": 2 n[v] + longest + 5 steps, cut as chunk_pieces5 with v's own n;
    "window": n[v] + 1 steps, cut in front of n[v] - 1, n[v] and n[v] + 1; "chunk": chunk + 1 steps around the granule.
    -> {name: (totals, pieces per utterance)}"""
    assert no_own_index(MODEL5_IDS) and sorted(MODEL5_IDS) == sorted(list(range(5)) * 2)
    out = {}
    for name in ("long", "window", "chunk"):
        pieces = [chunk_pieces5(chunk, n[v], 2 * n[v] + longest + 5) if name == "long" else window_pieces(GRANULE5, n[v], n[v] + 1) if name == "window"
                  else [3, 1, 5, chunk + 1 - 9] for v in MODEL5_IDS]
        assert in_lockstep_per_voice(schedule_of(pieces), MODEL5_IDS)
        out[name] = ([sum(p) for p in pieces], pieces)
    return out
