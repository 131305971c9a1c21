"""The case table of tests/test_gpu_voices_matrix.py (GPU) and tests/test_voices_matrix_cases.py (CPU, which holds this
table to design-only plans): the several-voices variant of every shape of vtm_synth_kernel (the kernel's kVoicesFlag),
where it differs from the single-voice kernel -- utterances picked through the row map, groups that end with empty rows,
each workgroup on its voice's constants, wavetable and ring inside an LDS laid out for the longest ring of the launch, a
stream's own chunk argument and state stride.

A cell is precision {f64, mixed, f32} x tube (the five of shape_matrix_cases.TUBES) x mix x forced rows {1, 2, 4}: 135
cells.  The mix names the voices of the plan (in plan order) and which of the tube's two output rates they run at:

    up      male, female                 the tube's up rate     both up-sample: rings that follow the chunk
    mixed   male, female, baby           the tube's up rate     baby down-samples: the launch's LDS is laid out for its
                                                                1024-sample ring, male and female run their 256 / 512 in it
    down    male, female, large_child    the tube's down rate   all three down-sample (baby is refused at SectionDelay 4
                                                                and 22 050 Hz: below the supported down-sampling range)

113 cells launch with the rows forced on them; the 22 of VOICES_FALL_BACK, four rows with a 1024-sample ring in the
launch, exceed the 160 KB of LDS and launch as two rows.  A lockstep stream keeps each voice's one-row ring, with which
the cells of VOICES_STREAM_FALL_BACK launch as two rows too.  The library decides (gvtm_debug_launch_shape with voices,
gvtm_debug_stream_launch_shape); the tests hold both sets to its answers.

Launch A, per cell, at the 250 Hz control rate: voice v gets the nine frame counts shape_matrix_cases.frames_a(C,
steps_v, seed) -- 0, 1 and 2 frames, the three last-chunk residues of THAT voice's steps per frame, seeded lengths up to
48 -- on pool_tracks' tracks, C the chunk of the shape the launch takes.  Voices 0, 1 and 2 get 9, 10 and 11 utterances
(the extra ones repeat the voice's longest members), so the last group of a voice holds 1 / 2 / 3 utterances of four rows
(3 / 2 / 1 rows empty) and 1 / 2 / 1 of two (1 / 0 / 1 empty); a seeded permutation shuffles the batch of 19 or 30.
Launch B, on the same plan: seven utterances none of which uses voice 0 (its group list is empty, the next voice starts at
group 0), one id -1 and one id n_voices.  The stream: rows + 1 utterances per voice in lockstep, one full group and one
partly empty group each."""
import collections
import ctypes
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import gama_tts_amd as g
from gama_tts_amd import capi
import oracle
import tracks
from shape_matrix_cases import POOL, PRECISIONS, ROWS, STREAM_FRAMES, TUBES, chunk_length, frames_a, hooks, pool_tracks
from voice_cases import configs, oracle_config

# mix -> (voices in plan order, index into the tube's rates, gvtm_plan_voice_info(...).upsampling per voice)
MIXES = collections.OrderedDict([
    ("up", (("male", "female"), 0, (1, 1))),
    ("mixed", (("male", "female", "baby"), 0, (1, 1, 0))),
    ("down", (("male", "female", "large_child"), 1, (0, 0, 0))),
])
BATCH_B = 7
SENTINEL = 7.0  # what the device outputs of the GPU tests start out as

Cell = collections.namedtuple("Cell", "pname precision delay layout mix names rate rows")
LaunchA = collections.namedtuple("LaunchA", "params ids frames member pools")
LaunchB = collections.namedtuple("LaunchB", "params bad_ids good_ids frames")


def tube_id(delay, layout):
    return "wide" if layout else "d%d" % delay


def cell_id(cell):
    return "%s-%s-%s-rows%d" % (cell.pname, tube_id(cell.delay, cell.layout), cell.mix, cell.rows)


CELLS = tuple(Cell(pname, precision, delay, layout, mix, names, tube["rates"][rate], rows)
              for pname, precision in PRECISIONS for (delay, layout), tube in TUBES.items()
              for mix, (names, rate, _) in MIXES.items() for rows in ROWS)
# four rows with a 1024-sample ring in the launch that do not fit the LDS: they launch as two rows (SectionDelay 3 keeps
# four rows in every precision, the float 48-lane tube too; every `up` cell keeps its rows)
VOICES_FALL_BACK = frozenset("%s-%s-%s-rows4" % (p, t, mix) for mix in ("mixed", "down")
                             for p, tubes in (("f64", ("d1", "d2", "d4", "wide")), ("mixed", ("d1", "d2", "d4", "wide")), ("f32", ("d1", "d2", "d4")))
                             for t in tubes)
LAUNCHABLE = tuple(c for c in CELLS if cell_id(c) not in VOICES_FALL_BACK)
# A stream keeps every voice's one-row ring: 512 samples when up-sampling, where the four-row shape's own is 256.  Of the
# launchable cells the lockstep streams of these seven launch as two rows (gvtm_debug_stream_launch_shape's answers): four
# rows of `up` in fp64 and float (not in mixed, nor with SectionDelay 3, nor the float 48-lane tube), the cells
# shape_matrix_cases.STREAM_FALL_BACK names for one voice.  106 of the 113 shapes run as streams of several voices.
VOICES_STREAM_FALL_BACK = frozenset(["f64-%s-up-rows4" % t for t in ("d1", "d2", "d4", "wide")] + ["f32-%s-up-rows4" % t for t in ("d1", "d2", "d4")])


def seed_of(cell):
    return 20000 + 40 * CELLS.index(cell)


def upsampling_of(cell):
    return MIXES[cell.mix][2]


def rows_of(cell):
    """The rows the cell's one-shot launch takes: its own, or two for the cells of VOICES_FALL_BACK."""
    return 2 if cell_id(cell) in VOICES_FALL_BACK else cell.rows


def stream_rows(cell):
    """The rows the cell's lockstep stream launches with: its own, or two for the cells of VOICES_STREAM_FALL_BACK."""
    return 2 if cell_id(cell) in VOICES_STREAM_FALL_BACK else cell.rows


def voices_plan(cell, device=0, rows=None):
    """The cell's plan of several voices with its rows forced (rows: others instead)."""
    return g.VoicesPlan(configs(cell.rate, cell.delay, cell.precision, cell.layout, names=cell.names), 250.0, device,
                        diagnostics=True, rows=cell.rows if rows is None else rows)


def single_plan(cell, voice, rows, device=0):
    """A single-voice plan of voice `voice` of the cell, `rows` forced."""
    return g.Plan(configs(cell.rate, cell.delay, cell.precision, cell.layout, names=[cell.names[voice]])[0], 250.0, device,
                  diagnostics=True, rows=rows)


def voices_launch_shape(plan, batch):
    """(rows, ring, LDS bytes) of a gvtm_synthesize_voices_* launch of `batch` utterances (gvtm_debug_launch_shape)."""
    out = (ctypes.c_size_t * 3)()
    rc = hooks().gvtm_debug_launch_shape(plan._h, batch, 1, out)
    assert rc == 0, rc
    return int(out[0]), int(out[1]), int(out[2])


def stream_launch_shape(plan, batch):
    """The same of a launch of a stream of the plan's voices pushed in lockstep (gvtm_debug_stream_launch_shape)."""
    out = (ctypes.c_size_t * 3)()
    rc = hooks().gvtm_debug_stream_launch_shape(plan._h, batch, out)
    assert rc == 0, rc
    return int(out[0]), int(out[1]), int(out[2])


@functools.lru_cache(maxsize=None)
def chunk_of(cell):
    """The chunk length of the shape the cell's voices launch takes: that of a single-voice design-only plan forced to
    the launched rows (the chunk follows precision, tube and rows, which the voices share)."""
    plan = single_plan(cell, 0, rows_of(cell), capi.DEVICE_NONE)
    try:
        return chunk_length(plan)
    finally:
        plan.close()


def batch_a(cell):
    return sum(POOL + v for v in range(len(cell.names)))


def utterances_per_voice(cell):
    return [POOL + v for v in range(len(cell.names))]


def empty_rows(count, rows):
    """Rows left empty in the last group of a voice with `count` utterances."""
    return (-count) % rows


# ---- inputs ----

def _stack(members, pools):
    """[(voice, pool member)] -> (params [B][F][16] zero beyond each frame count, frame counts)."""
    frames = np.array([pools[v][1][t] for v, t in members], dtype=np.int32)
    params = np.zeros((len(members), max(int(frames.max()), 1), 16), np.float32)
    for b, (v, t) in enumerate(members):
        params[b, : frames[b]] = pools[v][0][t, : frames[b]]
    return params, frames


def launch_a(cell, plan):
    """Launch A of the cell on `plan` (a device or design-only voices plan of it): params, ids, frame counts, the (voice,
    pool member) of every utterance and the pools [(tracks [POOL][..][16], frame counts [POOL])] per voice."""
    chunk, seed = chunk_of(cell), seed_of(cell)
    members, pools = [], []
    for v in range(len(cell.names)):
        fr = frames_a(chunk, int(plan.voice_info(v).control_steps), seed + 10 * v)
        pools.append((pool_tracks(fr, seed + 10 * v), fr))
        longest = np.argsort(-fr, kind="stable")[:v]  # v extra utterances: copies of the voice's longest members
        members += [(v, t) for t in range(POOL)] + [(v, int(t)) for t in longest]
    members = [members[i] for i in np.random.default_rng(seed + 7).permutation(len(members))]
    params, frames = _stack(members, pools)
    return LaunchA(params, np.array([v for v, _ in members], dtype=np.int32), frames, members, pools)


def launch_b(cell, a):
    """Launch B from launch A's pools: seven utterances, none of voice 0, one id -1 and one id n_voices -> params, the ids
    with the two bad ones, the ids of the launch without them (the two utterances as the voice whose track they carry) and frame counts."""
    n = len(cell.names)
    good = np.array([1, 1, 1, 1, 1, 1, 1] if n == 2 else [2, 1, 1, 2, 2, 1, 2], dtype=np.int32)
    bad = good.copy()
    bad[[2, 4]] = [-1, n]
    picks = [3, 8, 4, 5, 6, 7, 2]  # residues and seeded lengths of the voice's pool, and its two-frame member
    params, frames = _stack([(int(v), t) for v, t in zip(good, picks)], a.pools)
    return LaunchB(params, bad, good, frames)


def stream_case(cell):
    """The cell's stream: stream_rows + 1 utterances of every voice, shuffled -> (params [B][STREAM_FRAMES][16], ids)."""
    n, per = len(cell.names), stream_rows(cell) + 1
    ids = np.random.default_rng(seed_of(cell) + 9).permutation(np.repeat(np.arange(n, dtype=np.int32), per)).astype(np.int32)
    return tracks.random_tracks(ids.size, STREAM_FRAMES, seed0=seed_of(cell) + 20, consonant_heavy=True), ids


# ---- the oracle ----

def oracle_many(cell, jobs, workers=8):
    """jobs: [(voice of the cell, track [F][16])] at 250 Hz -> the oracle's samples of each (a thread pool: the C
    restatement keeps no global state and ctypes releases the GIL)."""
    cfgs = [oracle_config(name, cell.rate, cell.delay, cell.layout, cell.precision) for name in cell.names]
    oracle.lib()
    with ThreadPoolExecutor(workers) as ex:
        return list(ex.map(lambda j: oracle.synthesize(cfgs[j[0]], j[1]), jobs))


def oracle_pools(cell, a):
    """{(voice, pool member): the oracle's samples} of launch A."""
    keys = [(v, t) for v in range(len(cell.names)) for t in range(POOL)]
    refs = oracle_many(cell, [(v, a.pools[v][0][t, : int(a.pools[v][1][t])]) for v, t in keys])
    return dict(zip(keys, refs))
