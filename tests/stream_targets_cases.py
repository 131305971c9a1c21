"""What the tests of the targets-fed streams share: the pieces a session is cut into, the rule of what a list may forget in
front of a step, restated literally (include/gama_vtm.h, gvtm_targets_apply_host_from), the lists written for the edges of
resuming, and seeded random lists.  An utterance is 16 lists of (steps, values), as in targets_cases.py."""
import numpy as np

from modification_cases import wide_values
from targets_cases import FRIC_BW, FRIC_CF


def pieces(n, total):
    """The step counts a session of `total` steps is cut into for a filter of n samples: 1, 11, 12, 13 (around the granule of
    12 steps), n - 1, n, n + 1 (around the window), then the rest; a shorter session ends inside them."""
    out, left = [], total
    for piece in (1, 11, 12, 13, n - 1, n, n + 1):
        if left <= 0:
            break
        out.append(min(piece, left))
        left -= out[-1]
    return out + ([left] if left > 0 else [])


def boundaries(n, total):
    """The first step of every piece of pieces(n, total)."""
    return [int(b) for b in np.cumsum([0] + pieces(n, total))[:-1]]


def forget(lists, s0, n, one_more=False):
    """The lists as they may stand in front of step s0: a point is dropped once its successor has step <= s0 - 1 - n, which
    keeps the last point at or before the window's far edge and everything after it.  one_more: that point goes too (one
    point too many -- what the rule must not allow)."""
    far, out = s0 - 1 - n, []
    for steps, values in lists:
        k = 0
        while k + 1 < len(steps) and steps[k + 1] <= far:
            k += 1
        if one_more and k < len(steps) and steps[k] <= far:
            k += 1
        out.append((list(steps[k:]), np.asarray(values[k:], dtype=np.float32)))
    return out


def edge_lists(n, total, seed=0):
    """16 lists for a session of `total` >= 3 n + 40 steps cut by pieces(n, total): every place where resuming can go wrong."""
    rng = np.random.default_rng([n, seed, 61])
    f32 = lambda *v: np.asarray(v, dtype=np.float32)  # noqa: E731
    b = boundaries(n, total)  # 0, 1, 12, 24, 37, n + 36, 2 n + 36, 3 n + 37
    assert len(b) == 8 and b[7] == 3 * n + 37
    third = list(range(0, total, max(n // 3, 1)))
    thirty = [b[5] + 3 + 7 * i for i in range(30)]  # thirty points inside one window, behind a boundary
    assert thirty[-1] - thirty[0] < n
    lists = [
        ([0], f32(-0.75)),                                                      # 0: a point at step 0 only
        ([], f32()),                                                            # 1: no point at all
        ([b[3], b[5], b[6]], f32(1.0, -2.0, 0.5)),                              # 2: points exactly at a piece's first step
        ([b[3] - 1, b[4] - 1, b[6] - 1], f32(2.0, 0.25, -1.5)),                 # 3: ... and at a piece's last step
        ([b[5] - n, b[6] - n, b[7] - n], f32(3.0, -1.0, 2.5)),                  # 4: exactly N before a boundary: the leave cursor moves on the piece's first step
        (third, wide_values(rng, len(third))),                                  # 5 (fricCF): six decades apart in one window
        (third[1:], wide_values(rng, len(third) - 1)),                          # 6 (fricBW): the same, without a point at step 0
        (thirty, rng.uniform(-2.0, 2.0, 30).astype(np.float32)),                # 7: thirty points inside one window
        ([0, 20, 60, n + 100], f32(1.0, 2.0, 3.0, -1.0)),                       # 8: where forgetting one point too many shows (FORGET)
        ([0, b[5] - n - 1, b[5] - n, b[5] - n + 1], f32(0.5, 1.5, -0.5, 4.0)),  # 9: around the far edge of a boundary
        ([0, 1, 11, 12, 13, 23, 24, 25], rng.uniform(-1.0, 1.0, 8).astype(np.float32)),  # 10: around the granule's multiples
        ([b[7], total - 1], f32(7.0, -7.0)),                                    # 11: the last piece's first and last step
    ]
    assert (FRIC_CF, FRIC_BW) == (5, 6)
    while len(lists) < 16:
        count = int(rng.integers(1, 13))
        steps = np.sort(rng.choice(np.arange(total), count, replace=False))
        lists.append(([int(s) for s in steps], rng.uniform(-3.0, 3.0, count).astype(np.float32)))
    return [([int(s) for s in steps], np.asarray(values, dtype=np.float32)) for steps, values in lists]


FORGET = 8  # the list of edge_lists on which the point at the far edge still matters


def random_lists(n, total, seed):
    """16 seeded lists over a session of `total` steps: none to twelve points each, some with wide values, some from step 0."""
    rng = np.random.default_rng([n, seed, 67])
    lists = []
    for _ in range(16):
        count = int(rng.integers(0, 13)) if rng.random() < 0.8 else 0
        steps = np.sort(rng.choice(np.arange(total), count, replace=False))
        if count and rng.random() < 0.4:
            steps[0] = 0
        steps = np.unique(steps)
        values = wide_values(rng, len(steps)) if rng.random() < 0.3 else rng.uniform(-3.0, 3.0, len(steps)).astype(np.float32)
        lists.append(([int(s) for s in steps], np.asarray(values, dtype=np.float32)))
    return lists


def slice_lists(lists, first, count):
    """The points of the steps [first, first + count), their steps counted from `first`: what a push of those steps is given."""
    out = []
    for steps, values in lists:
        keep = [i for i, s in enumerate(steps) if first <= s < first + count]
        out.append(([steps[i] - first for i in keep], np.asarray([values[i] for i in keep], dtype=np.float32)))
    return out
