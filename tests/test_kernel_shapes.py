"""The host-side answers about every synthesis kernel shape (CPU test: design-only plans, diagnostics library).

gvtm_debug_lds_bytes(plan, rows) is the LDS of a workgroup of `rows` utterances of a plan.  It follows from the shape's
chunk length, the form of its records and its ring length together, so one number per shape pins all three.
tests/golden/kernel_shapes.json holds that number, as recorded from a build of the commit the file names, for

    precision {f64, mixed, f32} x SectionDelay {1, 2, 3, 4} x output rate {44100, 22050} x rows {1, 2, 4, 8}
    on the 10 + 6 tube, the same with SectionDelay 1 on the 30 + 18 tube (the 48-lane layout), and model 5 rows {1, 2}

Where a launch does not have the forced rows' shape, the hook answers for the shape the launch really uses, and the
file holds no entry of its own for such a case -- the test holds it to the entry of the shape it becomes:

    eight rows on the 48-lane layout (a tube wavefront per utterance, four at most): the four-row shape
    eight rows in mixed or f64 (float only has them):                                  the four-row shape

(The recorded build answered the second family with the ONE-row shape's bytes and the float case of the first with
bytes of an eight-row shape that no launch starts; both answers were the query's own mapping, not the launch's.)

The rows a launch takes (by batch size, precision, forced rows, voices, and what fits the LDS) are held to the rule
DESIGN.md states, through gvtm_debug_launch_shape, which answers from the function every launch asks.

Refresh after a deliberate change of a shape with    python tests/test_kernel_shapes.py --write
tests/tools/lds_sizes.py prints the same enumeration in KB."""
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import gama_tts_amd as g  # noqa: E402
from gama_tts_amd import capi  # noqa: E402
from kernel_shape_cases import GOLDEN, ROWS, launched_rows, lds_bytes, plans  # noqa: E402


def test_lds_bytes_of_every_shape_are_the_recorded_ones():
    golden = json.load(open(GOLDEN))["lds_bytes"]
    now = lds_bytes()
    assert len(now) == 3 * (4 + 1) * 2 * 4 + 2
    wrong = []
    for (name, rows), got in now.items():
        want = golden["%s rows %d" % (name, launched_rows(name, rows))]
        print("%-36s rows %d %7d B (recorded %7d)" % (name, rows, got, want))
        if got != want:
            wrong.append((name, rows))
    assert not wrong, wrong


def expected_rows(name, batch, forced, voices, golden):
    """The row choice as DESIGN.md states it ("Where a shape is decided"), on the recorded LDS bytes."""
    if name == "model5":
        return 2 if forced == 2 and not voices else 1
    if forced in ROWS:
        rows = forced
    else:
        rows = 4 if batch > 512 else (2 if batch > 256 else 1)
        if not name.startswith("f32") and int(name.split()[2]) >= 3:  # mixed or f64 with SectionDelay >= 3
            rows = min(rows, 2)
    if voices:
        rows = min(rows, 4)
    rows = launched_rows(name, rows)
    while rows > 1 and golden["%s rows %d" % (name, rows)] > 160 * 1024:
        rows //= 2
    return rows


def test_rows_of_a_launch_follow_batch_size_precision_forced_rows_voices_and_lds():
    """gvtm_debug_launch_shape answers from the function every launch asks (synth_launch_shape): 1 row up to 256 utterances,
    2 up to 512, 4 above; mixed and f64 with SectionDelay >= 3 at most 2 unless forced; forced rows 1, 2, 4, and 8 in float
    only (otherwise 4); a launch of several voices at most 4, model 5's 1; model 5 one row, two only when forced; and half
    as many rows while the LDS of a workgroup exceeds 160 KB.  The LDS bytes of the chosen rows are the recorded ones."""
    golden = json.load(open(GOLDEN))["lds_bytes"]
    lib = g.load_library(diagnostics=True)
    halved = 0
    for name, config, model5 in plans():
        for forced in (0, 1, 2, 4, 8):
            plan = g.Plan(config, 250.0, capi.DEVICE_NONE, diagnostics=True, rows=forced)
            for batch in (1, 256, 257, 512, 513, 4096):
                for voices in (0, 1):
                    out = (ctypes.c_size_t * 3)()
                    assert lib.gvtm_debug_launch_shape(plan._h, batch, voices, out) == 0, (name, forced, batch, voices)
                    want = expected_rows(name, batch, forced, voices, golden)
                    assert out[0] == want, (name, forced, batch, voices, out[0], want)
                    assert out[2] == golden["%s rows %d" % (name, want)] <= 160 * 1024, (name, forced, batch, voices)
                    halved += forced in ROWS and not model5 and want < min(forced, 4)
            plan.close()
    assert halved  # the enumeration has shapes that do not fit (down-sampling plans carry 1024-sample rings)


if __name__ == "__main__":
    if "--write" in sys.argv:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
        dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain", "--", "gama_tts_amd", "include"], capture_output=True, text=True).stdout.strip()
        recorded = {"%s rows %d" % (name, rows): v for (name, rows), v in lds_bytes().items() if launched_rows(name, rows) == rows}
        json.dump({"_comment": "gvtm_debug_lds_bytes of every kernel shape (tests/test_kernel_shapes.py --write), recorded from a build of commit "
                               + commit + (" with local changes" if dirty else ""),
                   "lds_bytes": recorded}, open(GOLDEN, "w"), indent=1)
        print("wrote", GOLDEN, len(recorded), "shapes")
    else:
        for (name, rows), v in lds_bytes().items():
            print(name, "rows", rows, v)
