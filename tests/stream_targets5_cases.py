"""What the tests of the targets-fed model 5 streams share (gvtm_stream_push_targets_model5): the pieces a session is cut
into around the granule of FOUR steps -- model 5's serial stages work in blocks of four, where the models 0 to 4 have a granule
of 12 -- and the lists written for the edges of resuming, at the positions of stream_targets_cases.edge_lists but with values
model 5 can speak.  An utterance is 16 lists of (steps, values), as in targets_cases.py; the parameters are pitch, glotVol,
aspVol, fricVol, fricPos, fricCF, fricBW, r1..r8, velum."""
import numpy as np

from modification_cases import wide_values
from targets_cases import FRIC_BW, FRIC_CF

GRANULE = 4
ASP_VOL, FRIC_VOL, VELUM = 2, 3, 15  # where 0 is the lower end of the editor's range: a list may start without a point at step 0
RADII = tuple(range(7, 15))


def pieces5(chunk, n):
    """The step counts a session of 2 n + chunk + 5 steps is cut into: around the granule of 4, around the chunk, and a piece
    (n - 1 steps, from step 3 chunk + 13 on) in which the leave cursor first moves; then the rest."""
    out = [1, 3, 4, 5, chunk - 1, chunk, chunk + 1, n - 1, n - 2 * chunk - 7]
    assert sum(out) == 2 * n + chunk + 5 and min(out) > 0
    return out


def edge_pieces5(n, total):
    """The edge session's pieces, whatever the chunk: 1, 3, 4, 5 (around the granule), n - 1, n, n + 1 (around the window), the rest."""
    out = [1, 3, 4, 5, n - 1, n, n + 1]
    assert total > sum(out)
    return out + [total - sum(out)]


def edge_boundaries5(n, total):
    """The first step of every piece of edge_pieces5: 0, 1, 4, 8, 13, n + 12, 2 n + 12, 3 n + 13."""
    return [int(b) for b in np.cumsum([0] + edge_pieces5(n, total))[:-1]]


def edge_pieces5_at_chunk(chunk, n, total):
    """edge_pieces5 with three more cuts, in front of the steps chunk - 1, chunk and chunk + 1: every boundary of the edge
    session stays one, and pushes end one step short of a chunk of the launch, on it and one step past it.  (Pieces of about a
    chunk's SIZE are pieces5's; three of them do not fit a session of 3 n + 45 steps beside the three of the window's size.)"""
    cuts = sorted(set(edge_boundaries5(n, total)[1:]) | {chunk - 1, chunk, chunk + 1})
    assert 13 < chunk - 1 and chunk + 1 < n + 12
    return [int(p) for p in np.diff([0] + cuts + [total])]


def edge_lists5(n, total, seed=0):
    """16 lists for a session of `total` >= 3 n + 40 steps cut by edge_pieces5(n, total): every place where resuming can go
    wrong (the step positions of stream_targets_cases.edge_lists, the granule's multiples being 4 and 8 here), on values of a
    spoken utterance (targets_cases.spoken_lists' source).  Only the two kinds without a point at step 0 -- no point at all, a
    list that starts late -- hold a parameter at 0, and they sit on aspVol, fricVol and velum; wide values sit on fricCF and
    fricBW and are positive."""
    import tracks
    assert total >= 3 * n + 40 and (FRIC_CF, FRIC_BW) == (5, 6)
    rng = np.random.default_rng([n, seed, 71])
    track = tracks.random_track(12, 300 + seed, consonant_heavy=True)
    b = edge_boundaries5(n, total)
    assert len(b) == 8 and b[7] == 3 * n + 13
    thirty = [0] + [b[5] + 3 + 7 * i for i in range(30)]  # thirty points inside one window, behind a boundary
    assert thirty[-1] - thirty[1] < n
    third = list(range(0, total, max(n // 3, 1)))
    fifth = list(range(0, total, max(n // 5, 1) + 1))
    positions = {
        0: thirty,                                          # pitch: thirty points inside one window (f0 moves push by push)
        1: [0, b[4], b[5], b[6]],                           # glotVol: points exactly at a piece's first step
        ASP_VOL: [],                                        # no point at all
        FRIC_VOL: [b[7], total - 1],                        # starts late: the last piece's first and last step
        4: [0],                                             # fricPos: a point at step 0 only
        FRIC_CF: third,                                     # six decades apart in one window
        FRIC_BW: fifth,                                     # the same at other steps
        7: [0, b[4] - 1, b[5] - 1, b[6] - 1],               # r1: points exactly at a piece's last step
        8: [0, b[5] - n, b[6] - n, b[7] - n],               # r2: exactly N before a boundary: the leave cursor moves on the piece's first step
        9: [0, 20, 60, n + 100],                            # r3: where forgetting one point too many would show
        10: [0, b[5] - n - 1, b[5] - n, b[5] - n + 1],      # r4: around the far edge of a boundary
        11: [0, 3, 4, 5, 7, 8, 9],                          # r5: around the granule's multiples
        VELUM: [b[5], b[6] + 1],                            # starts late, on a piece's first step
    }
    for p in (12, 13, 14):                                  # r6..r8: seeded, from step 0
        count = int(rng.integers(2, 13))
        positions[p] = [0] + [int(s) for s in np.sort(rng.choice(np.arange(1, total), count, replace=False))]
    lists = []
    for p in range(16):
        steps = positions[p]
        if p in (FRIC_CF, FRIC_BW):
            values = np.abs(wide_values(rng, len(steps))) + np.float32(1.0e-3)
        else:
            # the column's values in turn; a list that starts late begins with the column's largest
            first = int(np.argmax(track[:, p])) if steps and steps[0] > 0 else 0
            values = track[(first + np.arange(len(steps))) % track.shape[0], p]
        lists.append(([int(s) for s in steps], np.asarray(values, dtype=np.float32)))
    return lists
