"""The cases of tests/golden/targets_golden.npz -- target lists for the 16 parameters run through the reference's
MovingAverageFilter<float> under the loop of the rule as the header states it (tests/golden/ref_targets_table.cpp) -- the
literal restatement of the rule in Python (a real ring of N np.float32, Python floats -- IEEE doubles, one rounding per
operation -- for the sum), and the lists the GPU tests speak.

Plans: modification_cases.PLANS by key, and "half50": the male voice at a tract length that gives 20 050 Hz, where
rate * 0.05 is 1002.5 exactly: the reference's std::round goes half away from zero, N = 1003, where numpy's and Python's
round (half to even) say 1002.  An utterance is (S, lists): S internal steps and 16 lists, each (steps, values)."""
import fractions
import hashlib

import numpy as np

import modification_cases
from modification_cases import wide_values

PLANS = dict(modification_cases.PLANS)
PLANS["half50"] = modification_cases.Plan(20050.0, 80)  # male, vocal_tract_length 17.486, offset 0: N 1003
HALF50_OVERRIDES = {"vocal_tract_length": 17.486, "vocal_tract_length_offset": 0.0}
RULE_PLANS = ("male", "female", "half50")  # the plans the host rule's cases run on
FRIC_CF, FRIC_BW = 5, 6  # pitch, glotVol, aspVol, fricVol, fricPos, fricCF, fricBW, r1..r8, velum
STEP_LIMIT = 2 ** 31 - 4096  # steps the kernels' 31-bit counter holds, the flush behind them


def filter_length(rate):
    """(size_t)roundf((float)rate * (float)50.0e-3): a float product, rounded half away from zero."""
    product = np.float32(rate) * np.float32(50.0e-3)
    return int(np.floor(np.float64(product) + 0.5))  # (exact: a float plus 0.5 in double)


def make_plan(key, device, **kwargs):
    """The plan of PLANS[key] on `device` (capi.DEVICE_NONE: design-only), one voice."""
    if key == "half50":
        from gama_tts_amd import capi
        from voice_cases import male_plan
        return male_plan(HALF50_OVERRIDES, precision=capi.PRECISION_F32, device=device, **kwargs)
    return modification_cases.make_plan(key, device)


# ---- the rule, restated ----

def status_of(n_steps, lists, offsets=None):
    """The status of one utterance, in gvtm_targets_apply_host's order.  offsets: a doctored offset table."""
    if n_steps < 0 or n_steps >= STEP_LIMIT:
        return 1
    if offsets is not None and (min(offsets) < 0 or any(b < a for a, b in zip(offsets, offsets[1:]))):
        return 2
    if any(not np.isfinite(np.float32(v)) for _, values in lists for v in values):
        return 3
    for steps, _ in lists:
        steps = [int(s) for s in steps]
        if any(s < 0 for s in steps) or any(b <= a for a, b in zip(steps, steps[1:])):
            return 4
    return 0


def apply_rule(lists, n_steps, n):
    """16 lists of (steps, values) -> (v float32 [S][16], status); a refused utterance gives zeros.  The window's loop with
    the filter's ring, literally."""
    status = status_of(n_steps, lists)
    if status:
        return np.zeros((max(n_steps, 0), 16), np.float32), status
    out = np.zeros((n_steps, 16), dtype=np.float64)
    inv_n = 1.0 / n
    for p, (steps, values) in enumerate(lists):
        steps, values = [int(s) for s in steps], [np.float32(v) for v in values]
        nxt, cur = 0, np.float32(0.0)
        ring, pos, total = [np.float32(0.0)] * n, n, 0.0
        for s in range(n_steps):
            if nxt < len(steps) and steps[nxt] == s:
                cur = values[nxt]
                nxt += 1
            pos += 1
            if pos >= n:
                if pos > n:  # the first call
                    ring = [cur] * n
                    total = float(cur) * float(n)
                pos = 0
            total = total - float(ring[pos])
            total = total + float(cur)
            ring[pos] = cur
            out[s, p] = total * inv_n
    return out.astype(np.float32), 0  # (float)(sum * invN): one rounding, to nearest even


def _nearest_float32(q):
    c = np.float32(float(q))
    best = min((c, np.nextafter(c, np.float32(np.inf)), np.nextafter(c, np.float32(-np.inf))), key=lambda x: abs(fractions.Fraction(float(x)) - q))
    return np.float32(best)


def exact_mean_column(steps, values, n_steps, n):
    """What one list would give if v were the exactly rounded mean of the window (the last n values fed, the value fed at
    step 0 in front of it) -> float32 [S]."""
    steps, values = [int(s) for s in steps], [fractions.Fraction(float(np.float32(v))) for v in values]
    fed = []
    cur, nxt = fractions.Fraction(0), 0
    for s in range(n_steps):
        if nxt < len(steps) and steps[nxt] == s:
            cur, nxt = values[nxt], nxt + 1
        fed.append(cur)
    out = np.zeros(n_steps, np.float32)
    total = fed[0] * n if fed else 0
    for s in range(n_steps):
        total += fed[s] - (fed[s - n] if s >= n else fed[0])
        out[s] = _nearest_float32(total / n)
    return out


# ---- cases ----

def standard_lists(n, n_steps, seed):
    """16 lists for a filter of n samples and an utterance of n_steps steps: every kind of list the rule distinguishes."""
    rng = np.random.default_rng([n, seed, 50])
    f32 = lambda *v: np.asarray(v, dtype=np.float32)  # noqa: E731
    every = [int(s) for s in np.cumsum(rng.integers(2, 4, 90))]  # more than 64 points, one every 2 to 3 steps
    # wide_values' first run of four (the largest decade) at the first steps, so that the first call fills the ring with it;
    # then a point every n / 3 steps: the run of the smallest decade is 4 n / 3 steps long and has the window to itself once
    # the large values have left, with what they cost it in low bits
    third = [0, 1, 2, 3] + list(range(n // 8, 2 * n + 7, max(n // 3, 1)))
    edge = [s for s in (n_steps - 1, n_steps, n_steps + 1) if s >= 0]
    lists = [
        ([], f32()),                                                       # 0: empty: held at 0
        ([n // 3], f32(1.5)),                                              # 1: starts late
        ([0], f32(-0.75)),                                                 # 2: only a point at step 0
        ([5, 5 + n // 2], f32(2.0, -1.0)),                                 # 3: two changes less than N apart
        ([7, 7 + n], f32(0.25, 8.0)),                                      # 4: exactly N apart: both cursors move at one step
        ([40, 41, 42, 45, 46, 47], f32(1.0, -2.0, 3.0, 0.5, 0.25, 0.125)),  # 5: three changes inside one block of four steps, twice
        (edge, rng.uniform(1.0, 2.0, len(edge)).astype(np.float32)),      # 6: points at S - 1, S and S + 1
        (every, rng.uniform(-1.0, 1.0, len(every)).astype(np.float32)),    # 7: a long list
        (third, wide_values(rng, len(third))),                             # 8: six decades apart in one window
        ([0, 1, 2, 3], f32(4.0, 3.0, 2.0, 1.0)),                           # 9: a change at every one of the first steps
        ([0, n - 1, n, n + 1, 2 * n, 2 * n + 1], rng.uniform(-3.0, 3.0, 6).astype(np.float32)),  # 10: at the window's own edges
        ([3], f32(-0.0)),                                                  # 11: the sign of zero
        ([2 ** 31 - 1], f32(3.0e38)),                                      # 12: the last step an int32 holds
    ]
    while len(lists) < 16:
        count = int(rng.integers(1, 9))
        steps = np.sort(rng.choice(np.arange(2 * n + 20), count, replace=False))
        lists.append(([int(s) for s in steps], rng.uniform(-3.0, 3.0, count).astype(np.float32)))
    return [([int(s) for s in steps], np.asarray(values, dtype=np.float32)) for steps, values in lists]


WIDE = 8  # the list of standard_lists that holds wide_values


def _cases():
    out = {}
    for key in RULE_PLANS:
        n = filter_length(PLANS[key].rate)
        sizes = {"s0": 0, "s1": 1, "s200": 200, "nm1": n - 1, "n": n, "np1": n + 1, "2n7": 2 * n + 7}
        for name, n_steps in sizes.items():
            if key == "male" or name in ("s1", "s200", "np1", "2n7"):
                out["%s__%s" % (key, name)] = (key, n_steps, len(out))
    return out


CASES = _cases()  # name -> (plan key, S, seed)


def case(name):
    """-> (plan key, S, 16 lists)"""
    key, n_steps, seed = CASES[name]
    return key, n_steps, standard_lists(filter_length(PLANS[key].rate), n_steps, seed)


def random_case(seed):
    """A fresh case for the restatement against the host entry: (plan key, S, lists, doctored offsets or None).  About one in
    four breaks a rule (statuses 1 to 4); the rest are valid."""
    rng = np.random.default_rng([seed, 17])
    key = RULE_PLANS[seed % 3]
    n = filter_length(PLANS[key].rate)
    n_steps = int(rng.choice([0, 1, 2, 5, n // 7, n // 2, n + 3, n + n // 5]))
    lists = []
    for p in range(16):
        count = int(rng.integers(0, 7)) if rng.random() < 0.6 else 0
        steps = np.sort(rng.choice(np.arange(n_steps + 30), count, replace=False))
        values = wide_values(rng, count) if rng.random() < 0.3 else rng.uniform(-3.0, 3.0, count).astype(np.float32)
        if count and rng.random() < 0.4:
            steps[0] = 0
        lists.append(([int(s) for s in np.unique(steps)], values[: len(np.unique(steps))]))
    kind, offsets = int(rng.integers(0, 16)), None
    filled = [p for p in range(16) if len(lists[p][0]) >= 2]
    if kind == 0:
        n_steps = (-1, -n_steps - 1, STEP_LIMIT, 2 ** 40)[seed % 4]
    elif kind == 1:
        offsets = [int(o) for o in np.cumsum([0] + [len(l[0]) for l in lists])]
        p = int(rng.integers(1, 16))
        offsets[p] = (-1, offsets[p + 1] + 1)[seed % 2]
    elif kind == 2 and filled:
        p = filled[0]
        lists[p][1][int(rng.integers(0, len(lists[p][1])))] = (np.nan, np.inf, -np.inf)[seed % 3]
    elif kind == 3 and filled:
        p = filled[-1]
        steps = list(lists[p][0])
        steps[1] = (steps[0], -steps[1] - 1)[seed % 2]
        lists[p] = (steps, lists[p][1])
    return key, n_steps, lists, offsets


# ---- the lists the GPU tests speak ----

def spoken_lists(n_steps, seed, stride=211, wide=False):
    """16 lists whose values are key values of a random utterance (tracks.random_track, consonant-heavy), one every `stride`
    + 3 p steps from step 0 on -- strides that are multiples of nothing in the kernel -- so that every parameter stays what
    the model can speak.  wide: fricCF and fricBW (positive frequencies whatever their size) take values six decades apart."""
    import tracks
    rng = np.random.default_rng([seed, 23])
    track = tracks.random_track(max(n_steps // stride + 2, 2), seed, consonant_heavy=True)
    lists = []
    for p in range(16):
        steps = list(range(0, max(n_steps, 1) + 5, stride + 3 * p))
        values = track[np.arange(len(steps)) % track.shape[0], p].astype(np.float32)
        if wide and p in (FRIC_CF, FRIC_BW):
            steps = list(range(0, max(n_steps, 1) + 5, stride // 3 + p))
            values = np.abs(wide_values(rng, len(steps))) + np.float32(1.0e-3)
        lists.append((steps, values))
    return lists


# ---- the fixture ----

def sha256_of_inputs(rate, n_steps, lists):
    h = hashlib.sha256(np.asarray([rate], dtype="<f8").tobytes() + np.asarray([n_steps], dtype="<i8").tobytes())
    for steps, values in lists:
        h.update(np.asarray([len(steps)], dtype="<i4").tobytes())
        h.update(np.asarray(steps, dtype="<i4").tobytes())
        h.update(np.asarray(values, dtype="<f4").tobytes())
    return h.hexdigest()


def sha256_of_frames(frames):
    return hashlib.sha256(np.ascontiguousarray(frames, dtype="<f4").tobytes()).hexdigest()


FULL_ARRAY_STEPS = 256  # the fixture keeps the whole [S][16] array of a case up to this many steps


def check_frames(fixture, name, frames):
    """frames float32 [S][16] against the reference's for case `name`, bit for bit.  None if they match, else a message."""
    key, n_steps, lists = case(name)
    if bytes(fixture[name + "__inputs"]).decode() != sha256_of_inputs(PLANS[key].rate, n_steps, lists):
        return "%s: the fixture was made from other inputs (run tests/golden/make_targets_golden.py)" % name
    if frames.shape != (n_steps, 16):
        return "%s: %s, expected %s" % (name, frames.shape, (n_steps, 16))
    if n_steps <= FULL_ARRAY_STEPS:
        diff = frames.view(np.uint32) != fixture[name + "__frames"].view(np.uint32)
        if diff.any():
            bad = np.argwhere(diff)
            return "%s: %d values differ, first at step %d parameter %d" % (name, bad.shape[0], bad[0][0], bad[0][1])
    if bytes(fixture[name + "__sha256"]).decode() != sha256_of_frames(frames):
        return "%s: the frames' SHA-256 differs from the reference's" % name
    return None
