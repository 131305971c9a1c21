"""The ragged copy of a listening stream without a GPU: that the batches of tests/listen_copy_cases.py reach every path of
listen_copy_kernel (csrc/vtm_listen.hip), and listen_move of csrc/vtm_listen.hpp (gvtm_debug_listen_move of the diagnostics
library) against integer arithmetic at the ring's edges."""
import numpy as np
import pytest

import listen_copy_cases as lc
from gama_tts_amd import capi


def test_the_product_batch_reaches_every_path_of_the_kernel():
    batch = lc.product_batch()
    lc.check_coverage(*lc.paths(batch))  # (with 16-byte aligned arrays, as device allocations are)
    assert batch.max_len == 65536 and batch.src_stride % 2 == 1 and batch.dst_stride % 2 == 1
    assert set(batch.len.tolist()) == set(lc.LENGTHS) | {-1}
    assert (batch.len == 0).sum() > 16 and (batch.len == -1).sum() >= 8
    for off, stride in ((batch.src_off, batch.src_stride), (batch.dst_off, batch.dst_stride)):
        assert set((off % 4).tolist()) == {0, 1, 2, 3}
        assert set(((np.arange(off.size) * stride) % 4).tolist()) == {0, 1, 2, 3}  # the row bases' alignments
    # the full product: every length at every pair of addresses modulo 4 samples
    b = np.arange(batch.len.size)
    rows = set(zip(batch.len.tolist(), ((b * batch.src_stride + batch.src_off) % 4).tolist(), ((b * batch.dst_stride + batch.dst_off) % 4).tolist()))
    assert rows >= {(n, s, d) for n in lc.LENGTHS for s in range(4) for d in range(4)}


def test_the_runs_of_a_batch_do_not_touch():
    for batch in (lc.product_batch(), lc.many_rows_batch()):
        for flat, off, stride in ((batch.src, batch.src_off, batch.src_stride), (batch.dst, batch.dst_off, batch.dst_stride)):
            start = np.arange(off.size) * stride + off
            end = start + np.maximum(batch.len, 0)
            assert start[0] >= lc.GAP and end[-1] + lc.GAP <= flat.size
            assert (start[1:] - end[:-1] >= lc.GAP).all()
        want = lc.expected(batch)
        assert (want != lc.SENTINEL).sum() == np.maximum(batch.len, 0).sum()  # (the source holds no sentinel)


def test_the_many_rows_batch_reaches_the_stride_over_y():
    batch = lc.many_rows_batch()
    assert batch.len.size == lc.MAX_Y + 5 and batch.max_len == 9 and set(batch.len.tolist()) == set(range(10))
    assert (batch.len[lc.MAX_Y:] > 0).all()
    seen, _ = lc.paths(batch)
    assert {s[0] for s in seen} == {"16", "4"}
    assert batch.src.nbytes + batch.dst.nbytes < 16 << 20


FILLS = [0, 1, 65535]


@pytest.mark.parametrize("fill", FILLS)
def test_listen_move_is_integer_arithmetic(fill):
    room = lc.RING - fill
    for n in (0, 1, room - 1, room, room + 1, room + 65536, 2 * 65536 + 3):
        m = capi.debug_listen_move(fill, n)
        total = fill + n
        assert (m["buffers"], m["fill_after"]) == (total // lc.RING, total % lc.RING) == capi.listen_buffer_count(fill, n), (fill, n)
        assert m["head_len"] == min(n, room) and m["inside_first"] == room, (fill, n)
        if m["buffers"] >= 1:
            assert m["tail_src"] == room + (m["buffers"] - 1) * lc.RING and m["tail_len"] == n - m["tail_src"] == m["fill_after"], (fill, n)
            assert m["head_len"] + lc.RING * (m["buffers"] - 1) + m["tail_len"] == n, (fill, n)
        else:
            assert m["tail_src"] == 0 and m["tail_len"] == 0 and m["head_len"] == n == m["fill_after"] - fill, (fill, n)
