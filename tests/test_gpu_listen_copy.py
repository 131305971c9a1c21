"""listen_copy_kernel (csrc/vtm_listen.hip) called alone through gvtm_debug_listen_copy of the diagnostics library, against
numpy slicing: the batches of tests/listen_copy_cases.py, the whole destination compared bit for bit, and the paths the
kernel took worked out from the addresses the device gave the arrays."""
import numpy as np
import pytest

import listen_copy_cases as lc
from gama_tts_amd import capi
from device_io import to_device, to_host

pytestmark = pytest.mark.gpu


def copy_on_device(batch):
    """-> (the destination after gvtm_debug_listen_copy, the paths taken at the device's addresses)"""
    d_src, d_dst, d_src_off, d_dst_off, d_len = to_device(batch.src, batch.dst, batch.src_off, batch.dst_off, batch.len)
    assert d_src.data_ptr() % 4 == 0 and d_dst.data_ptr() % 4 == 0
    capi.debug_listen_copy(d_src, batch.src_stride, d_dst, batch.dst_stride, d_src_off, d_dst_off, d_len, batch.len.size, batch.max_len)
    out, src_after = to_host(d_dst, d_src)
    assert np.array_equal(src_after, batch.src)
    return out, lc.paths(batch, d_src.data_ptr(), d_dst.data_ptr())


def compare(out, batch):
    want = lc.expected(batch)
    wrong = np.flatnonzero(out.view(np.uint32) != want.view(np.uint32))
    if wrong.size:
        start = np.arange(batch.len.size) * batch.dst_stride + batch.dst_off
        rows = np.searchsorted(start, wrong[:8], side="right") - 1
        detail = [(int(i), int(r), int(i - start[r]), int(batch.len[r]), float(out[i]), float(want[i])) for i, r in zip(wrong[:8], rows)]
        raise AssertionError("%d samples differ; (index, row, index in the row's run, the row's len, got, want): %s" % (wrong.size, detail))


def test_every_alignment_and_length_bit_for_bit_with_the_gaps_untouched():
    batch = lc.product_batch()
    out, (seen, behind) = copy_on_device(batch)
    lc.check_coverage(seen, behind)
    compare(out, batch)


def test_rows_beyond_the_grids_y_limit():
    batch = lc.many_rows_batch()
    out, (seen, _) = copy_on_device(batch)
    assert batch.len.size > lc.MAX_Y and {s[0] for s in seen} == {"16", "4"}
    compare(out, batch)


def test_a_batch_with_nothing_to_copy_leaves_the_destination():
    batch = lc.pack([(b % 4, (b + 1) % 4, -1 if b % 2 else 0) for b in range(9)], 37, 43, 48)
    assert batch.max_len == 0
    for max_len in (0, 4097):  # no launch at all, and a grid whose every workgroup exits
        out, _ = copy_on_device(batch._replace(max_len=max_len))
        compare(out, batch)
