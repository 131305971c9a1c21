"""What tests/test_listen_copy_cpu.py and tests/test_gpu_listen_copy.py share: the batches of the ragged copy of a listening
stream (launch_listen_copy, csrc/vtm_listen.hip) called alone, their numpy reference, and which of the kernel's paths a
batch takes, worked out from its addresses.

A batch is two flat float32 arrays and three int64 tables.  Row b's run of len[b] samples lies at src[b * src_stride +
src_off[b] ..] and goes to dst[b * dst_stride + dst_off[b] ..].  The strides are small and odd, so the row bases cycle through
the four alignments; the offsets then place every run where the table wants its address modulo 16 bytes, runs packed one
behind the other with at least GAP samples between two of them and around all of them.  The source holds distinct values
(its own indices), the destination a sentinel, and the whole destination is compared bit for bit: a write in front of a run,
behind it or into another row's gap shows."""
import collections
import itertools

import numpy as np

RING = 65536
CHUNK = 4096  # samples per workgroup (kCopyChunk)
MAX_Y = 65535  # the grid's y limit (kCopyMaxY)
GAP = 8  # samples that stay sentinel around a run: more than a peel of 3 that is not clamped, or a rest one too long, can reach
SENTINEL = np.float32(-7.5)
LENGTHS = [0, 1, 2, 3, 4, 5, 7, 8] + list(range(4093, 4101)) + [8191, 8192, 8193, 65536]

Batch = collections.namedtuple("Batch", "src dst src_stride dst_stride src_off dst_off len max_len")


def pack(rows, src_stride, dst_stride, slot):
    """rows: (source address class, destination address class, len) per row, the classes in samples modulo 4 relative to the
    arrays' bases -> Batch.  Every run takes at least `slot` samples of either array, so that the offsets stay >= 0 under
    the strides."""
    assert src_stride % 2 == 1 and dst_stride % 2 == 1 and slot >= max(src_stride, dst_stride)
    offs = {"s": [], "d": []}
    ends = {}
    for key, column in (("s", 0), ("d", 1)):
        at = GAP
        for b, row in enumerate(rows):
            at = max(at, b * slot + GAP)
            at += (row[column] - at) % 4
            offs[key].append(at)
            at += max(int(row[2]), 0) + GAP
        ends[key] = at + GAP
    lens = np.asarray([r[2] for r in rows], dtype=np.int64)
    b = np.arange(len(rows), dtype=np.int64)
    src_off, dst_off = np.asarray(offs["s"], dtype=np.int64) - b * src_stride, np.asarray(offs["d"], dtype=np.int64) - b * dst_stride
    assert (src_off >= 0).all() and (dst_off >= 0).all()
    src = np.arange(ends["s"], dtype=np.float32)
    assert ends["s"] < 2 ** 24  # (every index is a float of its own)
    dst = np.full(ends["d"], SENTINEL, dtype=np.float32)
    return Batch(src, dst, src_stride, dst_stride, src_off, dst_off, lens, int(max(lens.max(), 0)))


def product_batch():
    """The full product of the source's and the destination's address modulo 4 samples and LENGTHS, rows of length -1 and 0
    mixed in (their destination keeps the sentinel); max_len is the largest length, so most rows see chunks behind them."""
    rows = []
    for n, (n_len, s, d) in enumerate(itertools.product(LENGTHS, range(4), range(4))):
        rows.append((s, d, n_len))
        if n % 5 == 0:
            rows.append(((s + 1) % 4, d, -1 if n % 2 else 0))
    return pack(rows, 37, 43, 48)


def many_rows_batch():
    """MAX_Y + 5 rows of the lengths 0 to 9: the last five are reached by the stride over the grid's y."""
    rows = [(b % 4, (b // 4 + b // 16) % 4, b % 10) for b in range(MAX_Y + 5)]
    return pack(rows, 5, 7, 16)


def expected(batch):
    """The destination after the copy: numpy slicing on a copy of it."""
    out = batch.dst.copy()
    for b, n in enumerate(batch.len):
        if n > 0:
            s, d = b * batch.src_stride + batch.src_off[b], b * batch.dst_stride + batch.dst_off[b]
            out[d: d + n] = batch.src[s: s + n]
    return out


def paths(batch, src_base=0, dst_base=0):
    """What listen_copy_kernel does with each row that has samples, from the addresses (the arrays at the byte addresses
    src_base and dst_base): the set of (path, peel, rest, clamped) with path "16" or "4", peel and rest None on the 4-byte
    path, clamped whether the peel was cut at the row's length; and the number of rows with a chunk of the grid behind them."""
    seen, behind = set(), 0
    chunks = -(-batch.max_len // CHUNK)
    for b, n in enumerate(int(v) for v in batch.len):
        if n <= 0:
            continue
        behind += -(-n // CHUNK) < chunks
        sa = src_base + 4 * (b * batch.src_stride + int(batch.src_off[b]))
        da = dst_base + 4 * (b * batch.dst_stride + int(batch.dst_off[b]))
        if (sa ^ da) & 15:
            seen.add(("4", None, None, False))
            continue
        boundary = ((16 - (da & 15)) & 15) // 4
        peel = min(boundary, n)
        seen.add(("16", peel, (n - peel) % 4, boundary > n))
    return seen, behind


def check_coverage(seen, behind):
    """Both paths, every peel and every rest length, a clamped peel, and chunks that lie behind a row's length."""
    assert ("4", None, None, False) in seen
    vector = [s for s in seen if s[0] == "16"]
    assert {s[1] for s in vector} == {0, 1, 2, 3} and {s[2] for s in vector} == {0, 1, 2, 3}
    assert {(s[1], s[2]) for s in vector} >= set(itertools.product(range(4), range(4)))  # (and every pair of them)
    assert any(s[3] for s in vector)
    assert behind > 0
