"""The cases of tests/golden/modification_golden.npz -- base frames and parameter-modification gestures run through the
reference's MovingAverageFilter<float> under the loop of the rule as the header states it
(tests/golden/ref_modification_table.cpp) -- and the literal restatement of the rule in Python: the ring buffer, np.float32
for the floats, Python floats (IEEE doubles, one rounding per operation) for the sum, one gesture after the other.

Plans: the cases name a plan by key; PLANS holds the internal rate and the control steps the plan must report, so that the
fixture needs no library to be made and a test sees a plan that drifted.  "half" is the male voice at a tract length that
gives 22 125 Hz, where rate * 0.02 is 442.5 exactly: the reference's std::round goes half away from zero, N = 443, where
numpy's and Python's round (half to even) say 442.  (With one rounding rule the float and the double product agree on N for
every integer rate -- the fractions of rate / 50 are multiples of 0.02, and float(0.02) is off by 2.2e-8 of itself -- so the
rounding rule is the trap an integer rate can reach; filter_length() below is the float formula for all of them.)"""
import collections
import fractions
import hashlib
import zlib

import numpy as np

ADD, MULTIPLY = 0, 1
MAX_GESTURES = 64
R3, FRIC_VOL, VELUM, PITCH = 9, 3, 15, 0  # pitch, glotVol, aspVol, fricVol, fricPos, fricCF, fricBW, r1..r8, velum

Plan = collections.namedtuple("Plan", "rate cs")
PLANS = {
    "male": Plan(20034.0, 80),                # float, SectionDelay 1, 44.1 kHz, 250 Hz: N 401
    "female": Plan(23373.0, 93),              # N 467
    "half": Plan(22125.0, 88),                # male, vocal_tract_length 15.846, offset 0: N 443
    "male5": Plan(60411.42857142857, 242),    # model 5, double class: N 1208
    "male5f": Plan(60411.4296875, 242),       # model 5, float class (the rate is a float): N 1208
}
HALF_OVERRIDES = {"vocal_tract_length": 15.846, "vocal_tract_length_offset": 0.0}


def filter_length(rate):
    """(size_t)roundf((float)rate * (float)20.0e-3): a float product, rounded half away from zero."""
    product = np.float32(rate) * np.float32(20.0e-3)
    return int(np.floor(np.float64(product) + 0.5))  # (exact: a float plus 0.5 in double)


def make_plan(key, device):
    """The plan of PLANS[key] on `device` (capi.DEVICE_NONE: design-only), one voice."""
    from gama_tts_amd import capi
    from voice_cases import male_plan, model5_plan
    if key in ("male5", "male5f"):
        return model5_plan("male", float_class=key == "male5f", device=device)
    if key == "half":
        return male_plan(HALF_OVERRIDES, precision=capi.PRECISION_F32, device=device)
    import gama_tts_amd as g
    from voice_cases import configs
    return g.Plan(configs(precision=capi.PRECISION_F32, names=[key])[0], 250.0, device)


# ---- the rule, restated ----

def status_of(n_frames, gestures):
    """The status of one utterance, in gvtm_modification_apply_host's order."""
    if n_frames < 2:
        return 1
    if len(gestures) > MAX_GESTURES:
        return 2
    if any(not 0 <= p < 16 or op not in (ADD, MULTIPLY) for p, op, _, _ in gestures):
        return 3
    if any(not np.isfinite(np.float32(v)) for _, _, _, values in gestures for v in values):
        return 3
    for _, _, steps, _ in gestures:
        steps = [int(s) for s in steps]
        if any(s < 0 for s in steps) or any(b <= a for a, b in zip(steps, steps[1:])):
            return 4
    return 0


def apply_rule(frames, gestures, cs, n):
    """frames float32 [F][16], gestures [(parameter, operation, steps, values)] -> (modified frames, status); a refused
    utterance gives the frames back unchanged.  The processor's loop with the filter's ring, literally."""
    orig = np.ascontiguousarray(frames, dtype=np.float32).reshape(-1, 16)
    out = orig.copy()
    status = status_of(orig.shape[0], gestures)
    if status:
        return out, status
    inv_n = 1.0 / n
    for p, op, steps, values in gestures:
        steps, values = [int(s) for s in steps], [np.float32(v) for v in values]
        nxt, cur = 0, None
        ring, pos, total, first = [np.float32(0.0)] * n, n, 0.0, True
        for k in range(1, orig.shape[0]):
            for i in range(cs):
                s = (k - 1) * cs + i
                if nxt < len(steps) and steps[nxt] == s:
                    cur = values[nxt]
                    nxt += 1
                while nxt < len(steps) and steps[nxt] < s:  # (never: the steps increase; a list the status check let through)
                    nxt += 1
                if cur is None:
                    continue
                pos += 1
                if pos >= n:
                    if first:
                        ring = [cur] * n
                        total = float(cur) * float(n)
                        first = False
                    pos = 0
                total = total - float(ring[pos])
                total = total + float(cur)
                ring[pos] = cur
                fm = np.float32(total * inv_n)
                if i == 0:
                    out[k, p] = orig[k, p] + fm if op == ADD else orig[k, p] * fm
    return out, 0


def _nearest_float32(q):
    """A Fraction rounded to the nearest float32 (ties: whichever float() picks; no tie arises in the cases)."""
    c = np.float32(float(q))
    best = min((c, np.nextafter(c, np.float32(np.inf)), np.nextafter(c, np.float32(-np.inf))), key=lambda x: abs(fractions.Fraction(float(x)) - q))
    return np.float32(best)


def exact_mean_column(frames, gesture, cs, n):
    """What one gesture alone would write if fm were the exactly rounded mean of the window (the last n values fed, the
    first value in front of the first point) -> {frame: float32 value}."""
    orig = np.ascontiguousarray(frames, dtype=np.float32).reshape(-1, 16)
    p, op, steps, values = gesture
    steps, values = [int(s) for s in steps], [np.float32(v) for v in values]
    out = {}
    if not steps:
        return out
    for k in range(1, orig.shape[0]):
        s = (k - 1) * cs
        if s < steps[0]:
            continue
        total = fractions.Fraction(0)
        # the value fed at step x: the last point at or in front of it (the first value in front of the first point)
        edges = [s - n + 1] + [t for t in steps if s - n + 1 < t <= s] + [s + 1]
        for a, b in zip(edges, edges[1:]):
            fed = values[0]
            for t, v in zip(steps, values):
                if t <= a:
                    fed = v
            total += fractions.Fraction(float(fed)) * (b - a)
        fm = _nearest_float32(total / n)
        out[k] = orig[k, p] + fm if op == ADD else orig[k, p] * fm
    return out


# ---- cases ----

def base_frames(n_frames, seed):
    """Frames of both signs and many magnitudes (the apply entries do not care what a parameter means)."""
    rng = np.random.default_rng([seed, n_frames])
    return (rng.normal(0.0, 1.0, (n_frames, 16)) * 10.0 ** rng.integers(-2, 3, (n_frames, 16))).astype(np.float32)


def wide_values(rng, count):
    """Magnitudes from 1e-6 to 1e4 in runs of four points, both signs.  Every third run is of the largest decade and the
    run behind it of the smallest: while both are in the window the small values lose their low bits in the sum (more than
    53 bits apart), and once the large ones have left, what is left of the sum is not the sum of what is left."""
    runs = rng.uniform(-6.0, 4.0, (count + 3) // 4)
    runs[0::3], runs[1::3] = 3.5, -5.5
    exponents = np.repeat(runs, 4)[:count]
    return (rng.choice([-1.0, 1.0], count) * rng.uniform(1.0, 10.0, count) * 10.0 ** np.floor(exponents)).clip(-1.0e4, 1.0e4).astype(np.float32)


def _every(first, stride, end):
    return list(range(first, end, max(stride, 1)))


def _templates(cs, n):
    """name -> (frames, seed of the base, gestures) for a plan of cs steps per frame and a filter of n samples."""
    rng = np.random.default_rng([cs, n, 5])
    end40 = 39 * cs
    t = {
        "f2_step0": (2, [(R3, ADD, [0], [0.5])]),
        "f2_mid": (2, [(R3, ADD, [cs // 2], [0.5])]),                      # acts, and writes no frame
        "f3_mid": (3, [(R3, ADD, [cs // 2], [-0.75]), (VELUM, MULTIPLY, [1, 2, 5, cs - 1, cs], [2.0, 0.5, 3.0, -1.0, 1.5])]),
        "f3_last_step": (3, [(R3, ADD, [cs, 2 * cs - 1], [0.25, 8.0]), (FRIC_VOL, ADD, [2 * cs - 1], [1.0])]),
        "f3_beyond": (3, [(R3, ADD, [3, 2 * cs, 2 * cs + 7], [1.0, 2.0, 3.0]), (VELUM, ADD, [2 * cs, 5 * cs], [1.0, 2.0]), (PITCH, ADD, [], [])]),
        "hold": (40, [(R3, ADD, [3], [1.25])]),                               # held for more than 3 n steps: the jump
        "hold_two": (40, [(R3, MULTIPLY, [2 * cs + 5, 2 * cs + 5 + min(4 * n, end40 - 3 * cs - 5)], [1.1, 0.9])]),
        "half_n": (40, [(R3, ADD, _every(7, n // 2, end40), rng.uniform(-1.0, 1.0, len(_every(7, n // 2, end40))).astype(np.float32))]),
        "in_one_frame": (40, [(R3, ADD, [5 * cs + 1, 5 * cs + 2, 5 * cs + 3, 5 * cs + cs // 2, 6 * cs - 1], [1.0, -1.0, 0.5, 0.25, 2.0])]),
        "past_end": (40, [(R3, ADD, [10 * cs, end40 - 1, end40, end40 + 1, end40 + 10 * cs], [1.0, 2.0, 3.0, 4.0, 5.0]),
                          (VELUM, MULTIPLY, [end40, end40 + 5], [0.0, 2.0]), (FRIC_VOL, MULTIPLY, [], [])]),
        "mul_zero_neg": (40, [(FRIC_VOL, MULTIPLY, [0, 12 * cs + 3, 25 * cs], [0.0, -2.5, -0.0]), (R3, MULTIPLY, [4 * cs], [-0.0])]),
        "same_param": (40, [(R3, ADD, [10], [0.5]), (FRIC_VOL, MULTIPLY, [3 * cs + 1], [1.5]), (R3, ADD, [20 * cs + 3, 30 * cs], [-0.25, 0.125])]),
        "same_param_out_of_order": (40, [(R3, ADD, [5], [1.0]), (R3, MULTIPLY, [29 * cs - 1], [2.0]), (R3, ADD, [9 * cs, 9 * cs + n // 3], [3.0, -3.0]),
                                         (R3, ADD, [end40 + 1], [9.0]), (VELUM, ADD, [0], [0.125])]),
        "other_params": (17, [(p, p % 2, [p * cs // 2 + p], [0.5 + p / 8.0]) for p in range(16)]),
        "g64": (40, [(g % 16, (g // 16) % 2, _every((g * 37) % (30 * cs), n + 11 * g + 1, end40)[:6],
                      rng.uniform(-2.0, 2.0, len(_every((g * 37) % (30 * cs), n + 11 * g + 1, end40)[:6])).astype(np.float32)) for g in range(64)]),
        # (MULTIPLY keeps a relative difference of fm in the frame; behind ADD it can vanish in the base value)
        "wide": (40, [(R3, MULTIPLY, _every(2, n // 3, end40), wide_values(rng, len(_every(2, n // 3, end40)))),
                      (VELUM, ADD, _every(cs + 1, n // 5 + 1, end40), wide_values(rng, len(_every(cs + 1, n // 5 + 1, end40))))]),
        "wide_held": (40, [(PITCH, MULTIPLY, _every(0, n + 3, end40), wide_values(rng, len(_every(0, n + 3, end40))))]),
    }
    return {k: (f, zlib.crc32(k.encode()) % 1000, [(p, op, [int(s) for s in steps], np.asarray(v, dtype=np.float32)) for p, op, steps, v in gs])
            for k, (f, gs) in t.items()}


# which templates a plan takes (the male voice all of them)
_TAKES = {
    "male": None,
    "female": ("f3_mid", "hold", "half_n", "same_param", "wide"),
    "half": ("f2_step0", "hold", "half_n", "wide", "same_param_out_of_order"),
    "male5": ("f3_last_step", "hold", "hold_two", "half_n", "wide", "same_param"),
    "male5f": ("hold", "wide", "mul_zero_neg"),
}


def _cases():
    out = {}
    for key, plan in PLANS.items():
        templates = _templates(plan.cs, filter_length(plan.rate))
        for name in (_TAKES[key] or templates):
            out["%s__%s" % (key, name)] = (key,) + templates[name]
    return out


CASES = _cases()  # name -> (plan key, frames, seed of the base, gestures)


def case(name):
    """-> (plan key, base frames float32 [F][16], gestures)"""
    key, n_frames, seed, gestures = CASES[name]
    return key, base_frames(n_frames, seed), gestures


def random_case(seed):
    """A fresh case for the restatement against the host entry: (plan key, frames, gestures).  About one in four breaks a
    rule (statuses 1 to 4); the rest are valid."""
    rng = np.random.default_rng([seed, 91])
    key = ("male", "female", "half")[seed % 3]
    cs, n = PLANS[key].cs, filter_length(PLANS[key].rate)
    n_frames = int(rng.integers(2, 25))
    end = (n_frames - 1) * cs
    gestures = []
    for _ in range(int(rng.integers(0, 6))):
        count = int(rng.integers(0, 9))
        steps = np.sort(rng.choice(np.arange(end + 2 * cs), count, replace=False))
        values = wide_values(rng, count) if rng.random() < 0.3 else rng.uniform(-3.0, 3.0, count).astype(np.float32)
        if count and rng.random() < 0.3:
            values[rng.integers(0, count)] = 0.0
        gestures.append((int(rng.integers(0, 16)), int(rng.integers(0, 2)), [int(s) for s in steps], values))
    kind = int(rng.integers(0, 16))
    if kind == 0:
        n_frames = int(rng.integers(0, 2))
    elif kind == 1:
        gestures = [gestures[0] if gestures else (R3, ADD, [1], np.float32([1.0]))] * 65
    elif kind == 2 and gestures:
        gestures[-1] = ((16, -1)[seed % 2],) + gestures[-1][1:]
    elif kind == 3 and gestures and len(gestures[0][2]) >= 2:
        steps = list(gestures[0][2])
        steps[1] = steps[0]
        gestures[0] = gestures[0][:2] + (steps, gestures[0][3])
    return key, base_frames(n_frames, 5000 + seed), gestures


# ---- the fixture ----

def sha256_of(frames, gestures):
    """SHA-256 of a case's inputs: the frames, then per gesture its parameter, operation, steps and values."""
    h = hashlib.sha256(np.ascontiguousarray(frames, dtype="<f4").tobytes())
    for p, op, steps, values in gestures:
        h.update(np.asarray([p, op, len(steps)], dtype="<i4").tobytes())
        h.update(np.asarray(steps, dtype="<i4").tobytes())
        h.update(np.asarray(values, dtype="<f4").tobytes())
    return h.hexdigest()


def modified_parameters(gestures):
    return sorted({int(p) for p, _, _, _ in gestures})


def check_frames(fixture, name, frames):
    """frames float32 [F][16] against the reference's for case `name`, bit for bit: the columns the gestures name against
    the fixture's, every other column against the base.  Returns None if they match, else a message."""
    key, base, gestures = case(name)
    if bytes(fixture[name + "__sha256"]).decode() != sha256_of(base, gestures):
        return "%s: the fixture was made from other inputs (run tests/golden/make_modification_golden.py)" % name
    if frames.shape != base.shape:
        return "%s: %s frames, the base has %s" % (name, frames.shape, base.shape)
    columns = modified_parameters(gestures)
    want = base.copy()
    if columns:
        want[:, columns] = fixture[name + "__columns"]
    diff = frames.view(np.uint32) != want.view(np.uint32)
    if diff.any():
        bad = np.argwhere(diff)
        return "%s: %d values differ, first at frame %d parameter %d" % (name, bad.shape[0], bad[0][0], bad[0][1])
    return None
