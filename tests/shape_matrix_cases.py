"""The case table of tests/test_gpu_shape_matrix.py (GPU) and tests/test_shape_matrix_cases.py (CPU, which holds this
table to design-only plans): every shape of vtm_synth_kernel a launch can be forced to, and the inputs at which a chunked,
multi-row kernel goes wrong.

A cell is precision {f64, mixed, f32} x tube (SectionDelay 1 to 4 on the 10 + 6 tube, SectionDelay 1 on the 48-lane
layout) x the converter's direction (up: a ring that follows the chunk; down: the reference's 1024 samples) x forced rows
{1, 2, 4}, on the male voice: 90 cells.  79 launch with the rows that were forced; the 11 of FALL_BACK, four rows when
down-sampling, exceed the 160 KB of LDS with their 1024-sample rings and launch as the two-row shape, which is a cell of
its own.  launches(cell) asks the library; the tests hold FALL_BACK to its answer.  A stream keeps the one-row shape's
ring whatever shape it launches, and with that ring 7 more cells, STREAM_FALL_BACK, launch as two rows: 72 of the 79
shapes run as streams, the 7 repeat their two-row neighbours'.

The chunk length C of a cell comes from the diagnostics library (gvtm_debug_chunk_length), never from a number restated
here.  Two launches per cell, each a pool of POOL distinct tracks tiled to BATCH utterances (every track then sits in two
different DPP rows of a two- or four-row workgroup, and the last workgroup is partly empty):

    (a) control rate 250 Hz, s = 80 / 160 / 240 / 321 / 240 steps per frame: 0, 1 and 2 frames, the smallest frame counts
        that end on each of the residues of f * s modulo C this control rate can reach at its ends -- a whole last chunk,
        the shortest last chunk gcd(s, C) and the longest partial one C - gcd(s, C) --, the rest seeded lengths up to 48;
    (b) control rate = internal rate, one step per frame: 0, 1, C - 1, C, C + 1, 2C, 2C + 1, 3C - 1 frames and a seeded
        length below 3C: a whole last chunk, a one-step last chunk and one short by a step, with the 2 x pad flush zeros
        running over the following chunks."""
import collections
import ctypes

import numpy as np

import gama_tts_amd as g
from gama_tts_amd import capi
import tracks
from voice_cases import male_plan

PRECISIONS = (("f64", capi.PRECISION_F64), ("mixed", capi.PRECISION_MIXED), ("f32", capi.PRECISION_F32))
# (SectionDelay, tube layout) -> output rates (up-sampling, down-sampling), internal rate in Hz, steps per frame at 250 Hz
TUBES = collections.OrderedDict([
    ((1, 0), dict(rates=(44100.0, 16000.0), internal=20034, steps=80)),
    ((2, 0), dict(rates=(48000.0, 22050.0), internal=40068, steps=160)),
    ((3, 0), dict(rates=(96000.0, 22050.0), internal=60102, steps=240)),
    ((4, 0), dict(rates=(96000.0, 22050.0), internal=80137, steps=321)),
    ((1, 1), dict(rates=(96000.0, 22050.0), internal=60102, steps=240)),
])
DIRECTIONS = ("up", "down")
ROWS = (1, 2, 4)
POOL, BATCH = 9, 19
MAX_FRAMES_A = 48
STREAM_BATCH, STREAM_FRAMES, STREAM_PIECES = 5, 31, (1, 6, 2, 9, 1, 12)

Cell = collections.namedtuple("Cell", "pname precision delay layout direction rate rows")


def cell_id(cell):
    return "%s-%s-%s-rows%d" % (cell.pname, "wide" if cell.layout else "d%d" % cell.delay, cell.direction, cell.rows)


CELLS = tuple(Cell(pname, precision, delay, layout, direction, tube["rates"][DIRECTIONS.index(direction)], rows)
              for pname, precision in PRECISIONS for (delay, layout), tube in TUBES.items() for direction in DIRECTIONS for rows in ROWS)
# four rows of 1024-sample rings that do not fit the LDS: they launch as two rows
FALL_BACK = frozenset(["%s-%s-down-rows4" % (p, t) for p in ("f64", "mixed") for t in ("d1", "d2", "d4", "wide")]
                      + ["f32-%s-down-rows4" % t for t in ("d1", "d2", "d4")])
LAUNCHABLE = tuple(c for c in CELLS if cell_id(c) not in FALL_BACK)
# A stream keeps the one-row shape's ring for every shape.  When up-sampling that ring is 512 samples where the four-row
# shape's own is 256, and four rows of it exceed the LDS in fp64 and float (not in mixed, nor with SectionDelay 3, whose
# four-row chunk is shorter): the lockstep streams of these seven cells launch as two rows.
STREAM_FALL_BACK = frozenset(["f64-%s-up-rows4" % t for t in ("d1", "d2", "d4", "wide")] + ["f32-%s-up-rows4" % t for t in ("d1", "d2", "d4")])


def seed_of(cell):
    return 7000 + 10 * CELLS.index(cell)


def float_model(cell):
    return int(cell.precision == capi.PRECISION_F32)


def internal_rate(cell):
    return TUBES[cell.delay, cell.layout]["internal"]


def plan_of(cell, crate=250.0, device=0, rows=None):
    """The cell's plan with its rows forced (rows: others instead), every one from voice_cases.male_plan."""
    return male_plan(rate=cell.rate, delay=cell.delay, crate=crate, precision=cell.precision, layout=cell.layout,
                     rows=cell.rows if rows is None else rows, device=device)


def hooks():
    return g.load_library(diagnostics=True)


def launch_shape(plan, batch=BATCH):
    """(rows, ring, LDS bytes) of a one-shot launch of `batch` utterances of a plan, as gvtm_debug_launch_shape answers."""
    out = (ctypes.c_size_t * 3)()
    rc = hooks().gvtm_debug_launch_shape(plan._h, batch, 0, out)
    assert rc == 0, rc
    return int(out[0]), int(out[1]), int(out[2])


def stream_launch_shape(plan, batch=STREAM_BATCH):
    """The same of a launch of a stream whose `batch` utterances are pushed in lockstep (gvtm_debug_stream_launch_shape)."""
    out = (ctypes.c_size_t * 3)()
    rc = hooks().gvtm_debug_stream_launch_shape(plan._h, batch, out)
    assert rc == 0, rc
    return int(out[0]), int(out[1]), int(out[2])


def stream_rows(cell):
    """The rows the cell's lockstep stream launches with: its own, or two for the cells of STREAM_FALL_BACK."""
    return 2 if cell_id(cell) in STREAM_FALL_BACK else cell.rows


def chunk_length(plan, batch=BATCH):
    """Internal steps per tick of the kernel shape that launch takes (gvtm_debug_chunk_length)."""
    return int(hooks().gvtm_debug_chunk_length(plan._h, batch))


def launches(cell):
    """Whether a launch of a design-only plan with the cell's rows forced keeps them."""
    plan = plan_of(cell, device=capi.DEVICE_NONE)
    try:
        return launch_shape(plan)[0] == cell.rows
    finally:
        plan.close()


def oracle_job(cell, track, crate=250.0):
    """The cell's member of oracle.synthesize_many's job list."""
    return (track, cell.rate, cell.delay, cell.layout, float_model(cell), crate)


# ---- inputs ----

def residues(steps, chunk):
    """The lengths of a last chunk (0: a whole one) that launch (a) asks for: none, the shortest and the longest partial
    one a multiple of `steps` steps can leave within MAX_FRAMES_A frames.  On the male voice every cell reaches 0,
    gcd(steps, chunk) and chunk - gcd(steps, chunk); a voice whose steps per frame share no factor with a long chunk
    (187 steps, chunk 144) ends no utterance of up to 48 frames on a whole chunk and has the other two only."""
    reach = {(f * steps) % chunk for f in range(1, MAX_FRAMES_A + 1)}
    partial = reach - {0}
    return tuple(sorted(reach & {0}) + ([min(partial), max(partial)] if partial else []))


def _fill(out, n, draw):
    while len(out) < n:
        f = int(draw())
        if f not in out:
            out.append(f)
    return np.array(out, dtype=np.int32)


def frames_a(chunk, steps, seed):
    """Frame counts of launch (a)'s pool."""
    out = [0, 1, 2]
    for r in residues(steps, chunk):
        f = next(f for f in range(1, MAX_FRAMES_A + 1) if (f * steps) % chunk == r)
        if f not in out:
            out.append(f)
    rng = np.random.default_rng(seed)
    return _fill(out, POOL, lambda: rng.integers(3, MAX_FRAMES_A + 1))


def frames_b(chunk, seed):
    """Frame counts (= steps) of launch (b)'s pool."""
    rng = np.random.default_rng(seed + 1)
    return _fill([0, 1, chunk - 1, chunk, chunk + 1, 2 * chunk, 2 * chunk + 1, 3 * chunk - 1], POOL, lambda: rng.integers(2, 3 * chunk))


def pool_tracks(frames, seed):
    """[POOL][max frames][16]: consonant-heavy random tracks, every third one not, the longest tracks.edge_track; each cut
    to its frame count (zero beyond)."""
    n = max(int(frames.max()), 1)
    params = tracks.random_tracks(POOL, n, seed0=seed, consonant_heavy=True)
    params[::3] = tracks.random_tracks(len(params[::3]), n, seed0=seed + 500, consonant_heavy=False)
    edge = int(np.argmax(frames))
    params[edge, : frames[edge]] = tracks.edge_track(int(frames[edge]), seed)
    for t in range(POOL):
        params[t, frames[t]:] = 0.0
    return params


def tiled(pool_params, pool_frames):
    """The pool tiled to BATCH utterances -> (params, frame counts, pool member of each utterance)."""
    idx = np.arange(BATCH) % POOL
    return np.ascontiguousarray(pool_params[idx]), np.ascontiguousarray(pool_frames[idx]), idx


def stream_tracks(cell):
    """[STREAM_BATCH][STREAM_FRAMES][16] of the cell's stream."""
    return tracks.random_tracks(STREAM_BATCH, STREAM_FRAMES, seed0=seed_of(cell) + 5, consonant_heavy=True)
