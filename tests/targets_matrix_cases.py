"""The case table of tests/test_gpu_targets_matrix.py (GPU) and tests/test_targets_matrix_cases.py (CPU, which holds this
table to design-only plans): the targets variant (kTargetsFlag) of every shape of vtm_synth_kernel a launch can be forced
to, fed lists whose points sit ON the edges of the targets driver instead of off them.

Cells: those of shape_matrix_cases.py, plans at the 250 Hz control rate (the targets entries want an ordinary plan).  The
targets launch takes its rows where the frames launch takes them: gvtm_synthesize_targets_device builds a LaunchRequest with
`targets` set and launch_synthesis (csrc/vtm_capi_launch.cpp) asks plan->launch_shape(batch, rows, voices, 0, true, targets),
that is synth_launch_shape (csrc/vtm_kernels.hip), where `targets` is read in the model 5 branch only; launch_v2
(csrc/vtm_kernel_shapes.hpp) then instantiates the variant of the shape with the same U and C.  So gvtm_debug_launch_shape,
gvtm_debug_stream_launch_shape and gvtm_debug_chunk_length answer for a targets launch of the models 0 to 4 as they do for
a frames launch, the 79 / 11 and 72 / 7 splits are shape_matrix_cases', and the GPU test asserts rows and C from those hooks
in every case.  C always comes from gvtm_debug_chunk_length and N from plan.targets_filter_length(), never from a number here.

Step counts: a pool of POOL per cell -- 0, 1, C - 1, C, 2C + 1, N - 1, N + C + 2, 2N + 3 and one seeded length strictly
between C and N, drawn again until the pool holds all four residues modulo 4 (the driver walks blocks of four steps and a
partial last block runs on) -- tiled to BATCH utterances as shape_matrix_cases.tiled does.

Lists: edge_lists(C, N, n_steps, seed), 16 lists whose steps come from edge_steps: the chunk edges E = {kC - 1, kC, kC + 1,
kC + 3, kC + 4} (a point ENTERS there; kC, kC + 1 and kC + 3 share a block of four), their images E + N (with the point N
before it both cursors move at one step) and E - N (the point LEAVES on a chunk edge: a leave move lands on kC only from a
point at kC - N, so the set has these next to the images + N), and S - 1, S, S + 1 for the utterance's own S; cut to
n_steps + 5.  In every tick group of stage_interp (parameters 0 to 2, 3 to 6, 7 to 15) one list each carries

    A   kC - 1, kC, kC + 1, kC + 3 for a k inside the first chunks and one behind N; S - 1, S, S + 1
    B   jC - N and (j + 1)C - 1 - N for the first j with jC > N, and no point in the blocks of four of jC and (j + 1)C - 1
    C   kC and kC + N; k'C + u and k'C + w + N, u != w offsets of E that share a block of four behind N

and seeded points of the set beside them, 6 to 40 in all.  The rest: seeded subsets, the whole set (more than 64 points from
N + C steps on), a point at step 0 only, an empty list (velum 0).  Values are key values of a consonant-heavy
tracks.random_track, cycled; fricCF and fricBW take modification_cases.wide_values, positive.  Every list but the pitch's,
the fricVol's and the empty one has a point at step 0, so that no radius or frequency starts at 0.  coincidences() says
which of (a) to (f) of the module's GPU test the lists of a group reach, by looking at the lists alone.

A stream's lists also hold, on their A lists, the steps around every resume of its session (resume_edges: a launch begins
where the pushes have brought whole granules of 12 steps, not where a piece ends): b - 1 and b, and b - 1 - N and b - N.

Voices: the `mixed` mix of voices_matrix_cases.py (male + female + baby: both converter directions, three N), its cells and
its fall-back set; every utterance's lists are made with its own voice's N and the launch's C."""
import collections
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from gama_tts_amd import capi
import oracle
import tracks
import voices_matrix_cases as vm
from device_io import current_stream, filled, to_device, to_host
from modification_cases import wide_values
from shape_matrix_cases import BATCH, POOL
from stream_targets_cases import slice_lists  # noqa: F401 (the matrix tests cut their sessions with it)
from stream_targets_voices_cases import GRANULE
from targets_cases import FRIC_BW, FRIC_CF
from targets_io import GUARD
from voice_cases import oracle_config

GROUPS = ((0, 1, 2), (3, 4, 5, 6), tuple(range(7, 16)))  # stage_interp's tick offsets: Lp < 3, Lp < 7, the rest
LETTERS = "abcdef"
EDGE_OFFSETS = (-1, 0, 1, 3, 4)
ROLE_A, ROLE_B, ROLE_C = (0, 3, 7), (1, 4, 8), (2, 5, 9)
WHOLE, ONLY_STEP_0, EMPTY = 13, 14, 15
NO_STEP_0 = (0, 3, EMPTY)  # pitch and fricVol may start at 0
KEYS = 24  # key values per parameter, cycled
BAD_VOICE = 5
STREAM_BATCH = 5

VOICE_CELLS = tuple(c for c in vm.LAUNCHABLE if c.mix == "mixed")
VoicesCase = collections.namedtuple("VoicesCase", "utterances step_counts voice_ids bad")


# ---- step counts ----

def step_pool(C, N, seed):
    """The POOL step counts of a cell (the module's docstring)."""
    pool = [0, 1, C - 1, C, 2 * C + 1, N - 1, N + C + 2, 2 * N + 3]
    rng = np.random.default_rng([seed, 79])
    while True:
        s = int(rng.integers(C + 1, N))
        if s not in pool and len({x % 4 for x in pool + [s]}) == 4:
            return np.array(pool + [s], dtype=np.int32)


def tiled_steps(pool):
    """The pool tiled to BATCH utterances -> (step counts, pool member of each utterance)."""
    idx = np.arange(BATCH) % POOL
    return np.ascontiguousarray(pool[idx]), idx


def stream_total(C, N):
    return N + 3 * C + 70


def stream_pieces(C, N):
    """A resume in front of, on and behind a chunk edge and the window; the rest is 33 steps whatever the cell."""
    pieces = [1, 11, 13, C + 1, N - 1, 2 * C + 12]
    return pieces + [stream_total(C, N) - sum(pieces)]


def stream_bases(pieces):
    """The steps at which the launches of a session cut into `pieces` resume (tg_base > 0): a push launches when it brings
    the pending steps to a granule, and then whole granules; the finish launches what is pending."""
    pending, done, out = 0, 0, []
    for p in list(pieces) + [None]:
        launch = pending if p is None else (pending + p) // GRANULE * GRANULE
        pending = 0 if p is None else pending + p - launch
        if launch and done:
            out.append(done)
        done += launch
    return out


def resume_edges(bases, N):
    """The points a resume at step b can lose: the last one that entered and the first one that will (b - 1, b), the last one
    that left and the first one that will (b - 1 - N, b - N)."""
    return sorted({s for b in bases for s in (b - 1, b, b - 1 - N, b - N) if s >= 1})


# ---- lists ----

def edge_steps(C, N, n_steps, extra=()):
    """The steps the lists of an utterance of n_steps steps draw from, increasing; extra: a stream's resume_edges."""
    chunks = range(0, (n_steps + 5 + N) // C + 2)  # (far enough for the E - N that lie inside)
    edges = {k * C + d for k in chunks for d in EDGE_OFFSETS}
    steps = edges | {e + N for e in edges} | {e - N for e in edges if e - N >= 1} | {n_steps - 1, n_steps, n_steps + 1} | set(extra)
    return np.array(sorted(s for s in steps if 0 <= s <= n_steps + 5), dtype=np.int64)


def _block_pair(N):
    """Two offsets of E whose images + N share a block of four (C is a multiple of 4: whatever the chunk)."""
    return next((u, w) for u in EDGE_OFFSETS for w in EDGE_OFFSETS if u < w and (N + u) // 4 == (N + w) // 4)


def _roles(C, N, n_steps, seed):
    """-> (A's points, B's points, the steps B keeps free, C's points); the places depend on C, N and the seed alone, so
    that an utterance's lists are the beginning of a longer one's but for S - 1, S, S + 1."""
    rng = np.random.default_rng([C, N, seed, 73])
    j = -(-(N + 1) // C)  # the first chunk edge a leave move can sit on: j C - N >= 1
    a = [k * C + d for k in (int(rng.integers(1, 4)), j + int(rng.integers(1, 3))) for d in (-1, 0, 1, 3)]
    a += [s for s in (n_steps - 1, n_steps, n_steps + 1) if s >= 0]
    b = [j * C - N, (j + 1) * C - 1 - N]
    free = set(range(j * C, j * C + 4)) | set(range((j + 1) * C - 4, (j + 1) * C))
    kc, kd = (1, 2) if rng.random() < 0.5 else (2, 1)
    u, w = _block_pair(N)
    c = [kc * C, kc * C + N, kd * C + u, kd * C + w + N]
    return a, b, free, c


def edge_lists(C, N, n_steps, seed, extra=()):
    """16 lists of (steps, values) for an utterance of n_steps steps under chunk C and filter N (the module's docstring).
    extra: steps the A lists hold too (a stream's resume_edges)."""
    rng = np.random.default_rng([C, N, n_steps, seed, 71])
    pool = edge_steps(C, N, n_steps, extra)
    a, b, free, c = _roles(C, N, n_steps, seed)
    a = a + list(extra)
    track = tracks.random_track(17 * KEYS, seed, consonant_heavy=True)[::17]
    lists = []
    for p in range(16):
        if p == EMPTY:
            steps = []
        elif p == ONLY_STEP_0:
            steps = [0]
        elif p == WHOLE:
            steps = pool.tolist()
        else:
            must = a if p in ROLE_A else b if p in ROLE_B else c if p in ROLE_C else []
            must = sorted({s for s in must if s <= n_steps + 5} | (set() if p in NO_STEP_0 else {0}))
            rest = np.array([s for s in pool.tolist() if s not in must and not (p in ROLE_B and s in free)], dtype=np.int64)
            more = min(max(int(rng.integers(6, 41)) - len(must), 0), rest.size)
            steps = sorted(set(must) | set(rng.choice(rest, more, replace=False).tolist()))
        values = track[np.arange(len(steps)) % KEYS, p].astype(np.float32)
        if p in (FRIC_CF, FRIC_BW):
            values = np.abs(wide_values(rng, len(steps))) + np.float32(1.0e-3)
        lists.append(([int(s) for s in steps], np.asarray(values, dtype=np.float32)))
    return lists


def coincidences(lists, C, N, S):
    """Per tick group, which of these the lists of an utterance of S steps reach, as a string of letters.  A point at step
    0 is taken by the walk's beginning and never moves a cursor; a move counts inside the S steps only; a block of four is
    step // 4 (a one-shot launch walks from step 0, and C is a multiple of 4).
      a  a point enters at a step congruent to 0 modulo C, and one at a step congruent to C - 1
      b  a point leaves (its step + N) at a step congruent to 0 modulo C, and one congruent to C - 1, each with no point
         of its list in that block of four
      c  both cursors move at one step: two points exactly N apart
      d  both cursors move in one block of four at different steps
      e  three points enter inside one block of four
      f  points at S - 1, S and S + 1 (for S == 0: at S and S + 1)"""
    out = []
    for group in GROUPS:
        got = set()
        for p in group:
            points = np.asarray(lists[p][0], dtype=np.int64)
            has = set(points.tolist())
            enter = points[(points > 0) & (points < S)]
            leave = points[points > 0] + N
            leave = leave[leave < S]
            blocks = set((points // 4).tolist())
            got |= {"a%d" % r for r in (0, C - 1) if (enter % C == r).any()}
            got |= {"b%d" % r for r in (0, C - 1) if any(l % C == r and l // 4 not in blocks for l in leave.tolist())}
            if set(leave.tolist()) & set(enter.tolist()):
                got.add("c")
            if any(l // 4 == e // 4 and l != e for l in leave.tolist() for e in enter[enter // 4 == l // 4].tolist()):
                got.add("d")
            if enter.size and np.bincount(enter // 4).max() >= 3:
                got.add("e")
            if {S, S + 1} <= has and (S == 0 or S - 1 in has):
                got.add("f")
        whole = {"a": {"a0", "a%d" % (C - 1)}, "b": {"b0", "b%d" % (C - 1)}}
        out.append("".join(x for x in LETTERS if whole.get(x, {x}) <= got))
    return out


def pool_lists(C, N, pool, seed):
    """Every pool member's own lists."""
    return [edge_lists(C, N, int(s), seed + t) for t, s in enumerate(pool)]


def host_frames(plan, lists, n_steps, voice=0):
    """gvtm_targets_apply_host's frames: what the oracle and the frames entry are fed at one step per frame."""
    frames, status = capi.targets_apply_host(plan, lists, n_steps, voice=voice)
    assert status == 0, status
    return frames


# ---- voices ----

def voices_case(cell, plan):
    """Launch A of a cell of VOICE_CELLS on `plan` (a device or design-only voices plan of it): 7 / 6 / 6 utterances of the
    three voices, shuffled, each voice at the members of step_pool(C, N_v) that end on 2 N_v + 3, N_v + C + 2, C, N_v - 1,
    2C + 1, 0 (and the male voice's seeded one), each with edge_lists of its own N_v; and one more utterance, of voice
    id 3, at a seeded place."""
    C, seed = vm.chunk_of(cell), vm.seed_of(cell)
    members = []
    for v in range(3):
        N = plan.targets_filter_length(v)
        pool = step_pool(C, N, seed + 10 * v)
        members += [(v, N, int(pool[t])) for t in ([7, 6, 3, 5, 4, 0, 8] if v == 0 else [7, 6, 3, 5, 4, 0])]
    rng = np.random.default_rng(seed + 7)
    members = [members[i] for i in rng.permutation(len(members))]
    bad = int(rng.integers(0, len(members) + 1))
    members.insert(bad, (3, plan.targets_filter_length(0), C + 2))
    utterances = [edge_lists(C, N, s, seed + 100 + b) for b, (_, N, s) in enumerate(members)]
    return VoicesCase(utterances, [s for _, _, s in members], [v for v, _, _ in members], bad)


def oracle_voices(cell, plan, case, workers=8):
    """{b: the oracle's samples of utterance b under its voice, at one step per frame on the host rule's frames}."""
    cfgs = [oracle_config(name, cell.rate, cell.delay, cell.layout, cell.precision) for name in cell.names]
    rates = [plan.voice_info(v).internal_rate_hz for v in range(3)]
    for v in range(3):
        assert oracle.derive(cfgs[v], rates[v]).control_steps == 1
    good = [b for b, v in enumerate(case.voice_ids) if 0 <= v < 3]
    frames = [host_frames(plan, case.utterances[b], case.step_counts[b], case.voice_ids[b]) for b in good]
    oracle.lib()
    with ThreadPoolExecutor(workers) as ex:
        refs = list(ex.map(lambda i: oracle.synthesize(cfgs[case.voice_ids[good[i]]], frames[i], control_rate=rates[case.voice_ids[good[i]]]), range(len(good))))
    return dict(zip(good, refs))


# ---- the device ----

def run_frames(plan, frames, step_counts):
    """gvtm_synthesize_batch_device on a plan of one step per frame, frames[b] float32 [S_b][16] -> (audio that started out as
    GUARD bytes, counts, maxabs)."""
    batch, max_steps = len(step_counts), max(max(int(s) for s in step_counts), 1)
    params = np.zeros((batch, max_steps, 16), np.float32)
    for b, f in enumerate(frames):
        params[b, : f.shape[0]] = f
    stride = plan.output_capacity(max_steps)
    d_params, d_frames = to_device(params, np.asarray(step_counts, dtype=np.int32))
    d_audio, d_counts, d_maxabs = filled((batch, stride * 4), GUARD, np.uint8), filled(batch, -7, np.int64), filled(batch, 5.0, np.float32)
    plan.synthesize_device(d_params, batch, max_steps, d_audio, stride, d_frames, d_counts, d_maxabs, current_stream())
    audio, counts, maxabs = to_host(d_audio, d_counts, d_maxabs)
    return audio.view(np.float32).reshape(batch, stride), counts, maxabs

